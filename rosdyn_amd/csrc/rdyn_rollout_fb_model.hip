// rdyn_rollout_fb_model.hip -- closed-loop rollouts under a model-based law (rdyn_rollout_model_feedback): T steps of
//     x' = (dq, FD(q, dq, u - tau_c(q, dq) - tau_E(q, ext_t))),
//     computed torque        a = fma(kd, dq_ref[t] - dq, fma(kp, q_ref[t] - q, ddq_ref[t])),  u = clamp(tau_ff[t] + RNEA_m(q, dq, a))
//     gravity compensation   u = clamp(fma(kd, dq_ref[t] - dq, fma(kp, q_ref[t] - q, tau_ff[t])) + RNEA_m(q, 0, 0))
// RNEA_m the joint torque of the CONTROLLER's model of the arm (a chain of its own: other parameters, geometry or gravity than the
// plant's), swept inside the loop by rnea_eval (rdyn_model_law.h).
//   k_rollout_fb_model<NJ, INTEGRATOR, EXT>   k_rollout_fb's text (rdyn_rollout_body.inc with that kernel's hooks), the law replaced by
//     model_command: still ONE launch for the horizon, the state in registers.
//     Registers: the rule of rdyn_rollout_fb.hip -- one wave per SIMD, RK4 spills at 9 and 10 joints -- so nothing of the law lives
//     across an evaluation: under hold = 1 the command overwrites tau[] at the head of the step; under hold = 0 it is formed into rhs
//     immediately before the evaluation.  The model sweep reads the model's constants through the model's own pointer (scalar loads),
//     laundered once per law with the limits and the acceleration reference, and shares no transform with the plant's evaluation: its
//     registers are dead when the evaluation begins.
//     The law is a wave-uniform run-time choice: gravity compensation is the same sweep with v = a = 0 (has the
//     compiler's figures that decided it).
// Compiled once per integrator and wrench path (RDYN_FBM_VARIANT = integrator + 2 EXT) so that the four quarters build in parallel.
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
#include "rdyn_model_law.h"
#include "rdyn_launch_util.h"

#ifndef RDYN_FBM_VARIANT
#error "RDYN_FBM_VARIANT selects the integrator (bit 0) and the wrench path (bit 1) this object holds"
#endif
#if RDYN_FBM_VARIANT < 0 || RDYN_FBM_VARIANT > 3
#error "RDYN_FBM_VARIANT is 0 .. 3"
#endif
// (the preprocessor does not see the enumerators: the build hands over their values)
static_assert(RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER == 0 && RDYN_INTEGRATOR_RK4 == 1, "the Makefile names the integrators by these values");

namespace
{
template <int NJ, bool EXT>
__device__ __forceinline__ bool fbm_eval(ChainPtr c, const double (&q)[NJ], const double (&dq)[NJ], double (&rhs)[NJ], const ExtEval& xe)
{
  if constexpr (EXT)
    return fwd_dyn_eval_ext<NJ>(c, q, dq, rhs, xe);
  else
    return fwd_dyn_eval<NJ>(c, q, dq, rhs);
}

template <int NJ, int INTEGRATOR, bool EXT>
__global__ __launch_bounds__(64) void k_rollout_fb_model(const RdynRolloutModelFbArgs am)
{
  const RdynRolloutFbArgs& af = am.b;
  const RdynModelFeedbackArgs& mf = am.m;
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
      model_command<NJ>(c, fb, mf, off_fb, a.in_sj, t, q, dq, u);                                                               \
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
  if (!fb.hold) model_command<NJ>(c, fb, mf, off_fb, a.in_sj, t, q, dq, rhs);          \
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
#define RDYN_ROLLOUT_EVAL(c, q, dq, rhs) fbm_eval<NJ, EXT>(c, q, dq, rhs, xe)
#include "rdyn_rollout_body.inc"
#undef RDYN_ROLLOUT_EVAL
#undef RDYN_ROLLOUT_PREFETCH
#undef RDYN_ROLLOUT_TAKE
#undef RDYN_ROLLOUT_RHS
#undef RDYN_ROLLOUT_HEAD
}

template <int NJ>
hipError_t launch_rollout_fbm_nj(const RdynRolloutModelFbArgs& a, hipStream_t st)
{
  const RdynRolloutArgs& r = a.b.e.c.r;
  const size_t lds = r.staged ? (size_t)64 * (size_t)(r.n_active | 1) * 8 : 0;
  hipLaunchKernelGGL((k_rollout_fb_model<NJ, (RDYN_FBM_VARIANT & 1), (RDYN_FBM_VARIANT & 2) != 0>), dim3((unsigned)((r.n_samples + 63) / 64)),
                     dim3(64), lds, st, a);
  return hipGetLastError();
}
}  // namespace

#if RDYN_FBM_VARIANT == 0
#define RDYN_FBM_LAUNCH rdyn_launch_rollout_model_feedback_euler
#elif RDYN_FBM_VARIANT == 1
#define RDYN_FBM_LAUNCH rdyn_launch_rollout_model_feedback_rk4
#elif RDYN_FBM_VARIANT == 2
#define RDYN_FBM_LAUNCH rdyn_launch_rollout_model_feedback_ext_euler
#else
#define RDYN_FBM_LAUNCH rdyn_launch_rollout_model_feedback_ext_rk4
#endif

// one quarter: the caller (rdyn_launch_rollout_model_feedback below) has checked the arguments and chosen it
hipError_t RDYN_FBM_LAUNCH(int n_joints, const RdynRolloutModelFbArgs& a, hipStream_t st)
{
#define CALL(N) launch_rollout_fbm_nj<N>(a, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}

#if RDYN_FBM_VARIANT == 0
hipError_t rdyn_launch_rollout_model_feedback_rk4(int n_joints, const RdynRolloutModelFbArgs& a, hipStream_t st);
hipError_t rdyn_launch_rollout_model_feedback_ext_euler(int n_joints, const RdynRolloutModelFbArgs& a, hipStream_t st);
hipError_t rdyn_launch_rollout_model_feedback_ext_rk4(int n_joints, const RdynRolloutModelFbArgs& a, hipStream_t st);

hipError_t rdyn_launch_rollout_model_feedback(int n_joints, const RdynRolloutModelFbArgs& a, hipStream_t st)
{
  const RdynRolloutFbArgs& b = a.b;
  const RdynRolloutArgs& r = b.e.c.r;
  if (r.n_samples <= 0) return hipSuccess;
  if (r.integrator != RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER && r.integrator != RDYN_INTEGRATOR_RK4) return hipErrorInvalidValue;
  if (b.e.c.t.n_comps < 0 || b.e.c.t.n_comps > RDYN_MAX_COMPONENTS) return hipErrorInvalidValue;
  if (b.e.x.w && (b.e.x.one < 0 || b.e.x.one > n_joints + 1 || b.e.x.step < 0)) return hipErrorInvalidValue;
  if (!b.f.q_ref || !b.f.kp || b.f.ref_step < 0 || (b.f.hold | b.f.per_sample) & ~1) return hipErrorInvalidValue;
  if (!a.m.model || (a.m.law != RDYN_LAW_GRAVITY_COMPENSATION && a.m.law != RDYN_LAW_COMPUTED_TORQUE)) return hipErrorInvalidValue;
  if (a.m.law == RDYN_LAW_GRAVITY_COMPENSATION && a.m.ddq_ref) return hipErrorInvalidValue;
  const bool rk4 = r.integrator == RDYN_INTEGRATOR_RK4;
  if (b.e.x.w)
    return rk4 ? rdyn_launch_rollout_model_feedback_ext_rk4(n_joints, a, st) : rdyn_launch_rollout_model_feedback_ext_euler(n_joints, a, st);
  return rk4 ? rdyn_launch_rollout_model_feedback_rk4(n_joints, a, st) : rdyn_launch_rollout_model_feedback_euler(n_joints, a, st);
}
#endif
