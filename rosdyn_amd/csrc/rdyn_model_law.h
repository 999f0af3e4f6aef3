// rdyn_model_law.h -- the model-based laws of the closed-loop rollouts (rdyn_rollout_model_feedback): the controller's own model of the
// arm swept inside the loop.  rnea_eval is the ONE text of that sweep, written from the steps of rdyn_joint_step.h; model_command forms
// the command of either law with it and with the PD term of rdyn_feedback_law.h (k_rollout_fb_model, rdyn_rollout_fb_model.hip).
#ifndef RDYN_MODEL_LAW_H
#define RDYN_MODEL_LAW_H
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_joint_step.h"
#include "rdyn_feedback_law.h"

namespace
{
// tau = RNEA_m(q, v, a): what rdyn_joint_torque evaluates for the chain behind m -- its own geometry, parameters and gravity --, every
// vector by chain joint (joints that are no input joints rest at 0 and get 0).  The constants come through m by scalar loads where
// they are used; nothing but sin q / 1 - cos q and the net wrench of every link lives between the two passes, and the transforms are
// formed again on the way back, as the forward dynamics does.
template <int NJ>
__device__ __forceinline__ void rnea_eval(ChainPtr m, const double (&q)[NJ], const double (&v)[NJ], const double (&a)[NJ], double (&tau)[NJ])
{
  V3 w = mk(0, 0, 0), vl = mk(0, 0, 0), al = mk(0, 0, 0);
  V3 acc = mk(-m->g[0], -m->g[1], -m->g[2]);  // base "acceleration" -g
  double sv0[NJ], sv1[NJ];
  V3 Fo[NJ], No[NJ];
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    JointRef J = m->j[f];
    const bool act = J.in_idx >= 0;
    joint_sincos_state(J.type, act ? q[f] : 0.0, sv0[f], sv1[f]);
    double R[9];
    V3 t;
    joint_transform(J, sv0[f], sv1[f], R, t);
    primal_step(J, R, t, act ? v[f] : 0.0, act ? a[f] : 0.0, w, vl, al, acc);
    link_wrench(J, w, vl, al, acc, Fo[f], No[f]);
  }
  V3 F = mk(0, 0, 0), N = mk(0, 0, 0);
#pragma unroll
  for (int j = NJ - 1; j >= 0; --j)
  {
    JointRef J = m->j[j];
    F = F + Fo[j];
    N = N + No[j];
    const V3 u = ld3(J.u);
    double tj = 0.0;
    if (J.type == RDYN_REVOLUTE) tj = dot(u, N);
    else if (J.type == RDYN_PRISMATIC) tj = dot(u, F);
    tau[j] = J.in_idx >= 0 ? tj : 0.0;
    if (j == 0) break;
    // the wrench carried back into the parent's frame: x_parent = R x + t
    double R[9];
    V3 t;
    joint_transform(J, sv0[j], sv1[j], R, t);
    const V3 Fp = rot(R, F);
    N = rot(R, N) + cross(t, Fp);
    F = Fp;
  }
}

// the command of the lane's sample at step t and state (q, dq), by chain joint: u[f] holds tau_ff on entry.  c = the plant (the input
// indices; the model has the same ones, checked by the host), off / sj as in fb_command.
//   computed torque         a = fma(kd, dq_ref - dq, fma(kp, q_ref - q, ddq_ref)),  u = clamp(tau_ff + RNEA_m(q, dq, a))
//   gravity compensation    p = fma(kd, dq_ref - dq, fma(kp, q_ref - q, tau_ff)),   u = clamp(p + RNEA_m(q, 0, 0))
// One sweep serves both: the law is a wave-uniform choice of what enters it.  The PD terms are fb_law's text without its clamp, the
// loads those of fb_command_gains (PER_SAMPLE: the lane's own gains, vector loads; otherwise scalar loads by the input index).
template <int NJ, bool PER_SAMPLE>
__device__ __forceinline__ void model_command_gains(ChainPtr c, const RdynFeedbackArgs& fb, const RdynModelFeedbackArgs& mf, int64_t off, int64_t sj,
                                                    int t, const double (&q)[NJ], const double (&dq)[NJ], double (&u)[NJ])
{
  const bool ct = mf.law == RDYN_LAW_COMPUTED_TORQUE;  // wave-uniform
  const bool vel = fb.kd != nullptr;
  const int64_t at = (int64_t)t * fb.ref_step + off;
  // pointers laundered once per law (rdyn_rollout_fb.hip: nothing of the law is to be hoisted and carried across the evaluations)
  uint64_t r0 = (uint64_t)(fb.q_ref + at), r1 = (uint64_t)(fb.dq_ref ? fb.dq_ref + at : nullptr), r2 = (uint64_t)(mf.ddq_ref ? mf.ddq_ref + at : nullptr);
  uint64_t g0 = (uint64_t)fb.kp, g1 = (uint64_t)fb.kd, g2 = (uint64_t)fb.lim, pm = (uint64_t)mf.model;
  asm volatile("" : "+v"(r0), "+v"(r1), "+v"(r2));
  asm volatile("" : "+s"(g0), "+s"(g1), "+s"(g2), "+s"(pm));
  const double *const qr = (const double*)r0, *const dqr = (const double*)r1, *const ar = (const double*)r2;
  const double *const kp = (const double*)g0, *const kd = (const double*)g1, *const lim = (const double*)g2;
  const ChainPtr m = (ChainPtr)pm;
  double v[NJ], a[NJ];  // what enters the sweep; a first takes the PD sum: the model's acceleration, or (gravity compensation) the PD command
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    const int idx = c->j[f].in_idx;
    v[f] = ct ? dq[f] : 0.0;
    a[f] = 0.0;
    if (idx < 0) continue;
    const int64_t o = idx * sj;
    const int64_t g = PER_SAMPLE ? off + o : (int64_t)idx;
    const double dr = (vel && dqr) ? dqr[o] : 0.0;
    const double base = ct ? (ar ? ar[o] : 0.0) : u[f];
    a[f] = fb_law(base, qr[o], q[f], kp[g], vel, dr, dq[f], vel ? kd[g] : 0.0, false, 0.0);
  }
  double pd[NJ], mt[NJ];
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    pd[f] = ct ? u[f] : a[f];  // what the model torque is added to: tau_ff, or the PD command
    a[f] = ct ? a[f] : 0.0;
  }
  rnea_eval<NJ>(m, q, v, a, mt);
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    const int idx = c->j[f].in_idx;
    if (idx < 0) continue;
    double r = pd[f] + mt[f];
    if (lim)
    {
      const double l = lim[idx];
      r = r > l ? l : (r < -l ? -l : r);
    }
    u[f] = r;
  }
}

template <int NJ>
__device__ __forceinline__ void model_command(ChainPtr c, const RdynFeedbackArgs& fb, const RdynModelFeedbackArgs& mf, int64_t off, int64_t sj, int t,
                                              const double (&q)[NJ], const double (&dq)[NJ], double (&u)[NJ])
{
  if (fb.per_sample)  // wave-uniform
    model_command_gains<NJ, true>(c, fb, mf, off, sj, t, q, dq, u);
  else
    model_command_gains<NJ, false>(c, fb, mf, off, sj, t, q, dq, u);
}
}  // namespace
#endif
