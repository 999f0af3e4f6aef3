// rdyn_rollout_fb.hip -- closed-loop rollouts (rdyn_rollout_feedback): T steps of
//     x' = (dq, FD(q, dq, u - tau_c(q, dq) - tau_E(q, ext_t))),
//     u_j = clamp(fma(kd_j, dq_ref[t]_j - dq_j, fma(kp_j, q_ref[t]_j - q_j, tau_ff[t]_j)), +-lim_j)
// a joint-space PD law around the torque sequence of rdyn_rollout, which becomes the feed-forward term.  The clamp is two comparisons, so a
// NaN command stays NaN (fmin / fmax would turn it into a limit and hide the failure from the status).  hold = 1: the command is formed once
// per step from the state at the start of the step and held over the stages like tau_t (a digital controller); hold = 0: formed at every
// stage at the stage's own state (the continuous law), as the components are.
//   k_rollout_fb<NJ, INTEGRATOR, EXT>   k_rollout's text (rdyn_rollout_body.inc) with the law, the component subtraction of k_rollout_comp
//     and, for EXT, the wrench evaluation of k_rollout_ext: still ONE launch for the horizon, the state in registers.  EXT = false evaluates
//     with fwd_dyn_eval and carries nothing of the wrench path.
//     Registers: these kernels sit at one wave per SIMD and RK4 spills at 9 and 10 joints, so the law carries NOTHING across an
//     evaluation.  hold = 1 writes the command over the step's torques in tau[] at the head of the step (RDYN_ROLLOUT_HEAD): those
//     registers are not written again until the step's last evaluation has taken its copy.  The references, and per-sample gains, are
//     read where the law is formed -- 2 NJ (4 NJ) loads at the head of the step under hold = 1, the same again at each later stage under
//     hold = 0, where L2 serves them -- instead of being requested a step ahead (2 NJ more live doubles).  Shared gains and the limits are
//     indexed by the wave-uniform input index: scalar loads.  The pointers are laundered once per law (the per_evaluation concern of
//     rdyn_rollout_body.h: the loads are invariant over RK4's stage loop, the shared ones over the step loop, and hoisted they would be
//     carried in registers across the evaluations).
//     The command record of a step that is due (the command of the step's first evaluation: formed at the head of the step from the
//     start state under either mode, the same expression and so the same bits as stage 0 forms) leaves through put_record and
//     SmallRecords under the condition of the state records.
//   k_rollout_command   the chunked route: one thread per double, every access contiguous; forms u into one more state array of the
//     workspace, which the stage's forward-dynamics pass takes in place of tau_t (rdyn_api_dynamics.cpp), and writes the record that is due.
// Compiled once per integrator and wrench path (RDYN_FB_VARIANT = integrator + 2 EXT) so that the four quarters build in parallel.
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_record_stage.h"
#include "rdyn_fwd_dyn_body.h"
#include "rdyn_rollout_body.h"
#include "rdyn_component_row.h"
#include "rdyn_ext_wrench.h"
#include "rdyn_feedback_law.h"
#include "rdyn_launch_util.h"

#ifndef RDYN_FB_VARIANT
#error "RDYN_FB_VARIANT selects the integrator (bit 0) and the wrench path (bit 1) this object holds"
#endif
#if RDYN_FB_VARIANT < 0 || RDYN_FB_VARIANT > 3
#error "RDYN_FB_VARIANT is 0 .. 3"
#endif
// (the preprocessor does not see the enumerators: the build hands over their values)
static_assert(RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER == 0 && RDYN_INTEGRATOR_RK4 == 1, "the Makefile names the integrators by these values");

namespace
{
template <int NJ, bool EXT>
__device__ __forceinline__ bool fb_eval(ChainPtr c, const double (&q)[NJ], const double (&dq)[NJ], double (&rhs)[NJ], const ExtEval& xe)
{
  if constexpr (EXT)
    return fwd_dyn_eval_ext<NJ>(c, q, dq, rhs, xe);
  else
    return fwd_dyn_eval<NJ>(c, q, dq, rhs);
}

template <int NJ, int INTEGRATOR, bool EXT>
__global__ __launch_bounds__(64) void k_rollout_fb(const RdynRolloutFbArgs af)
{
  const RdynRolloutExtArgs& ax = af.e;
  const RdynRolloutArgs& a = ax.c.r;
  const RdynExtArgs& x = ax.x;
  const RdynFeedbackArgs& fb = af.f;
  // the lane's sample (lanes past the batch leave at the head of the body and read nothing)
  const int64_t s_fb = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool in_batch = s_fb < a.n_samples;
  const int64_t off_fb = (in_batch ? s_fb : 0) * a.in_ss;
  ExtEval xe;
  xe.rec = nullptr;
  xe.se = 0;
  xe.one = 0;
  xe.l = xe.a = mk(0, 0, 0);
  const double* xp = nullptr;
  V3 wl = mk(0, 0, 0), wa = mk(0, 0, 0);  // one link: the wrench of the step (of the next one once the evaluation has its copy)
  if constexpr (EXT)
  {
    xp = x.w + (in_batch ? s_fb : 0) * x.ss;
    xe.rec = xp;
    xe.se = x.se;
    xe.one = x.one;
    if (x.one && in_batch && a.n_steps > 0) ext_load6(xp, x.se, wl, wa);
  }
  // the head of step t: the command of the step's first evaluation, wanted when it is held or its record is due
#define RDYN_ROLLOUT_HEAD                                                                                                       \
  {                                                                                                                             \
    const bool rec_due = fb.tau_traj && a.traj_every > 0 && due == 1;                                                           \
    if (fb.hold || rec_due)                                                                                                     \
    {                                                                                                                           \
      double u[NJ];                                                                                                             \
      _Pragma("unroll") for (int f = 0; f < NJ; ++f) u[f] = tau[f];                                                             \
      fb_command<NJ>(c, fb, off_fb, a.in_sj, t, q, dq, u);                                                                      \
      if (fb.hold) { _Pragma("unroll") for (int f = 0; f < NJ; ++f) tau[f] = u[f]; }                                            \
      if (rec_due)                                                                                                              \
      {                                                                                                                         \
        _Pragma("unroll") for (int f = 0; f < NJ; ++f) u[f] = alive ? u[f] : qnan;                                              \
        put_record<NJ>(c, sm, stg_traj, u, fb.tau_traj + rec_off + s_wave * a.in_ss, fb.tau_traj + rec_off + s * a.in_ss, a.in_sj, lane); \
      }                                                                                                                         \
    }                                                                                                                           \
  }
  // immediately before each evaluation: the continuous law at the stage state, then the components behind the clamp
#define RDYN_ROLLOUT_RHS(q, dq, rhs)                                                   \
  if (!fb.hold) fb_command<NJ>(c, fb, off_fb, a.in_sj, t, q, dq, rhs);                 \
  _Pragma("unroll") for (int f = 0; f < NJ; ++f)                                       \
  {                                                                                    \
    const int idx = c->j[f].in_idx;                                                    \
    if (idx >= 0) rhs[f] -= joint_component_torque(ax.c.t, idx, q[f], dq[f]);          \
  }
#define RDYN_ROLLOUT_TAKE                            \
  if constexpr (EXT)                                 \
  {                                                  \
    if (x.one)                                       \
    {                                                \
      xe.l = wl;                                     \
      xe.a = wa;                                     \
    }                                                \
    else                                             \
      xe.rec = xp + (int64_t)t * x.step;             \
  }
#define RDYN_ROLLOUT_PREFETCH \
  if constexpr (EXT)          \
  {                           \
    if (x.one && x.step != 0) ext_load6(xp + (int64_t)(t + 1) * x.step, x.se, wl, wa); \
  }
#define RDYN_ROLLOUT_EVAL(c, q, dq, rhs) fb_eval<NJ, EXT>(c, q, dq, rhs, xe)
#include "rdyn_rollout_body.inc"
#undef RDYN_ROLLOUT_EVAL
#undef RDYN_ROLLOUT_PREFETCH
#undef RDYN_ROLLOUT_TAKE
#undef RDYN_ROLLOUT_RHS
#undef RDYN_ROLLOUT_HEAD
}

template <int NJ>
hipError_t launch_rollout_fb_nj(const RdynRolloutFbArgs& a, hipStream_t st)
{
  const RdynRolloutArgs& r = a.e.c.r;
  const size_t lds = r.staged ? (size_t)64 * (size_t)(r.n_active | 1) * 8 : 0;
  hipLaunchKernelGGL((k_rollout_fb<NJ, (RDYN_FB_VARIANT & 1), (RDYN_FB_VARIANT & 2) != 0>), dim3((unsigned)((r.n_samples + 63) / 64)), dim3(64), lds,
                     st, a);
  return hipGetLastError();
}

#if RDYN_FB_VARIANT == 0
// thread e: double e of the (contiguous) arrays; its sample is e / n (sample-major) or e % n_samples (element-major), its joint the other
__global__ __launch_bounds__(256) void k_rollout_command(const RdynRolloutCommandArgs a)
{
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.count) return;
  const int64_t s = a.element_major ? e % a.n_samples : e / a.n;
  const int64_t j = a.element_major ? e / a.n_samples : e % a.n;
  const int64_t g = a.per_sample ? e : j;
  const bool vel = a.kd != nullptr, clamp = a.lim != nullptr;
  const double dr = (vel && a.dq_ref) ? a.dq_ref[e] : 0.0;
  const double u = fb_law(a.tau_ff[e], a.q_ref[e], a.q[e], a.kp[g], vel, dr, a.dq[e], vel ? a.kd[g] : 0.0, clamp, clamp ? a.lim[j] : 0.0);
  a.u[e] = u;
  if (a.rec) a.rec[e] = a.st_run[s] < 0 ? __builtin_nan("") : u;
}
#endif
}  // namespace

#if RDYN_FB_VARIANT == 0
#define RDYN_FB_LAUNCH rdyn_launch_rollout_feedback_euler
#elif RDYN_FB_VARIANT == 1
#define RDYN_FB_LAUNCH rdyn_launch_rollout_feedback_rk4
#elif RDYN_FB_VARIANT == 2
#define RDYN_FB_LAUNCH rdyn_launch_rollout_feedback_ext_euler
#else
#define RDYN_FB_LAUNCH rdyn_launch_rollout_feedback_ext_rk4
#endif

// one quarter: the caller (rdyn_launch_rollout_feedback below) has checked the arguments and chosen it
hipError_t RDYN_FB_LAUNCH(int n_joints, const RdynRolloutFbArgs& a, hipStream_t st)
{
#define CALL(N) launch_rollout_fb_nj<N>(a, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}

#if RDYN_FB_VARIANT == 0
hipError_t rdyn_launch_rollout_feedback_rk4(int n_joints, const RdynRolloutFbArgs& a, hipStream_t st);
hipError_t rdyn_launch_rollout_feedback_ext_euler(int n_joints, const RdynRolloutFbArgs& a, hipStream_t st);
hipError_t rdyn_launch_rollout_feedback_ext_rk4(int n_joints, const RdynRolloutFbArgs& a, hipStream_t st);

hipError_t rdyn_launch_rollout_feedback(int n_joints, const RdynRolloutFbArgs& a, hipStream_t st)
{
  const RdynRolloutArgs& r = a.e.c.r;
  if (r.n_samples <= 0) return hipSuccess;
  if (r.integrator != RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER && r.integrator != RDYN_INTEGRATOR_RK4) return hipErrorInvalidValue;
  if (a.e.c.t.n_comps < 0 || a.e.c.t.n_comps > RDYN_MAX_COMPONENTS) return hipErrorInvalidValue;
  if (a.e.x.w && (a.e.x.one < 0 || a.e.x.one > n_joints + 1 || a.e.x.step < 0)) return hipErrorInvalidValue;
  if (!a.f.q_ref || !a.f.kp || a.f.ref_step < 0 || (a.f.hold | a.f.per_sample) & ~1) return hipErrorInvalidValue;
  const bool rk4 = r.integrator == RDYN_INTEGRATOR_RK4;
  if (a.e.x.w) return rk4 ? rdyn_launch_rollout_feedback_ext_rk4(n_joints, a, st) : rdyn_launch_rollout_feedback_ext_euler(n_joints, a, st);
  return rk4 ? rdyn_launch_rollout_feedback_rk4(n_joints, a, st) : rdyn_launch_rollout_feedback_euler(n_joints, a, st);
}

hipError_t rdyn_launch_rollout_command(const RdynRolloutCommandArgs& a, hipStream_t st)
{
  if (a.count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rollout_command, dim3((unsigned)((a.count + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}
#endif
