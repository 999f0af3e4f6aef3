// rdyn_rollout_adjoint_fb.hip -- the adjoint of a closed-loop rollout (rdyn_rollout_adjoint_feedback; no counterpart in the reference):
// the exact transpose of the scheme k_rollout_fb integrates.  k_rollout_adjoint_fb<NJ, INTEGRATOR, EXT> IS k_rollout_adjoint
// (rdyn_rollout_adjoint_body.inc, RDYN_ADJ_FB on; EXT: RDYN_ADJ_EXT on as well) with two hooks around every evaluation:
//   the command     before each rebuilt RK4 stage evaluation and before each product the law is formed again with the forward kernel's
//                   text (rdyn_feedback_law.h), so the product is taken at the bits of the command the forward call applied.  hold = 1
//                   and semi-implicit Euler: once, at the head of the step, over the step's torques in tau[]; hold = 0 with RK4: at every
//                   stage state, into the evaluation's copy.
//   the transpose   fb_transpose, ONE text for every path, after each product (hold = 0 with RK4) or after the step's products (hold = 1,
//                   Euler).  With tot = tau_bar_total + gu (gu: the seed on the step's command record, first evaluation only) and the
//                   raw command u_raw the law gives before the clamp:
//                       g    = (u_raw > lim || u_raw < -lim) ? +0.0 : tot                     a select, not a product
//                       q_bar = fma(-kp, g, q_bar)      v_bar = fma(-kd, g, v_bar)            (v_bar only with kd)
//                       gkp   = fma(q_ref - q, g, gkp)  gkd   = fma(dq_ref - dq, g, gkd)      glim += u_raw > lim ? tot : (u_raw < -lim ? -tot : +0.0)
//                   and g replaces tau_bar: it is the gradient with respect to the feed-forward torque and takes tau_bar's way into
//                   gtau.  The reference gradients of a step are kp * gtau_t and kd * gtau_t, formed once when the step is complete.
// Registers: the adjoint kernels spill from 4 - 5 joints and sit at one wave per SIMD, so the law carries NOTHING across an evaluation:
// references and per-sample gains are loaded where the law and its transpose are formed (laundered pointers, as k_rollout_fb does),
// shared gains and limits by the wave-uniform input index (scalar loads), the feed-forward torques of a held command are loaded again
// for the transpose, and gkp / gkd / glim / the summed reference gradients are accumulated in the lane's OWN output rows in memory:
// read-modify-write by the one lane that owns them, in the order of the backward sweep (gw's precedent in RDYN_ADJ_EXT).  No lane
// touches another's row and there are no atomics: the same bits every run, and the same bits however the horizon is split into chained
// calls (accumulate = 1 continues the additions where the later part left them).
// A sample that fails at a backward step -- a failed product, or a non-finite reference, gain or limit -- gets NaN in that step's
// reference gradients and every earlier one, and in its whole gkp / gkd / glim rows and summed reference gradients.
// Compiled once per integrator and wrench path (RDYN_ADJ_FB_VARIANT = integrator + 2 EXT) so that the four quarters build in parallel.
#include <hip/hip_runtime.h>
#include "rdyn_rollout_adjoint_body.h"
#include "rdyn_ext_wrench.h"
#include "rdyn_feedback_law.h"
#include "rdyn_feedback_transpose.h"
#include "rdyn_launch_util.h"

#ifndef RDYN_ADJ_FB_VARIANT
#error "RDYN_ADJ_FB_VARIANT selects the integrator (bit 0) and the wrench path (bit 1) this object holds"
#endif
#if RDYN_ADJ_FB_VARIANT < 0 || RDYN_ADJ_FB_VARIANT > 3
#error "RDYN_ADJ_FB_VARIANT is 0 .. 3"
#endif
// (the preprocessor does not see the enumerators: the build hands over their values)
static_assert(RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER == 0 && RDYN_INTEGRATOR_RK4 == 1, "the Makefile names the integrators by these values");

namespace
{
template <int NJ, int INTEGRATOR, bool EXT>
__global__ __launch_bounds__(64) void k_rollout_adjoint_fb(const RdynRolloutAdjointFbArgs af)
{
  const RdynRolloutAdjointExtArgs& ax = af.ax;
  const RdynRolloutAdjointArgs& a = ax.a;
  const RdynFeedbackArgs& fb = af.f;
  const RdynFeedbackGradArgs& gf = af.g;
  (void)ax;
#define RDYN_ADJ_PARAMS 0
#define RDYN_ADJ_EXT ((RDYN_ADJ_FB_VARIANT & 2) != 0)
#define RDYN_ADJ_FB 1
#include "rdyn_rollout_adjoint_body.inc"
#undef RDYN_ADJ_FB
#undef RDYN_ADJ_EXT
#undef RDYN_ADJ_PARAMS
}

template <int NJ>
hipError_t launch_adjoint_fb_nj(const RdynRolloutAdjointFbArgs& a, hipStream_t st)
{
  const RdynRolloutAdjointArgs& r = a.ax.a;
  const size_t lds = (r.staged || a.g.staged) ?(size_t)64 * (size_t)(r.n_active | 1) * 8 : 0;
  hipLaunchKernelGGL((k_rollout_adjoint_fb<NJ, (RDYN_ADJ_FB_VARIANT & 1), (RDYN_ADJ_FB_VARIANT & 2) != 0>), dim3((unsigned)((r.n_samples + 63) / 64)),
                     dim3(64), lds, st, a);
  return hipGetLastError();
}
}  // namespace

#if RDYN_ADJ_FB_VARIANT == 0
#define RDYN_ADJ_FB_LAUNCH rdyn_launch_rollout_adjoint_feedback_euler
#elif RDYN_ADJ_FB_VARIANT == 1
#define RDYN_ADJ_FB_LAUNCH rdyn_launch_rollout_adjoint_feedback_rk4
#elif RDYN_ADJ_FB_VARIANT == 2
#define RDYN_ADJ_FB_LAUNCH rdyn_launch_rollout_adjoint_feedback_ext_euler
#else
#define RDYN_ADJ_FB_LAUNCH rdyn_launch_rollout_adjoint_feedback_ext_rk4
#endif

// one quarter: the caller (rdyn_launch_rollout_adjoint_feedback below) has checked the arguments and chosen it
hipError_t RDYN_ADJ_FB_LAUNCH(int n_joints, const RdynRolloutAdjointFbArgs& a, hipStream_t st)
{
#define CALL(N) launch_adjoint_fb_nj<N>(a, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}

#if RDYN_ADJ_FB_VARIANT == 0
hipError_t rdyn_launch_rollout_adjoint_feedback_rk4(int n_joints, const RdynRolloutAdjointFbArgs& a, hipStream_t st);
hipError_t rdyn_launch_rollout_adjoint_feedback_ext_euler(int n_joints, const RdynRolloutAdjointFbArgs& a, hipStream_t st);
hipError_t rdyn_launch_rollout_adjoint_feedback_ext_rk4(int n_joints, const RdynRolloutAdjointFbArgs& a, hipStream_t st);

hipError_t rdyn_launch_rollout_adjoint_feedback(int n_joints, const RdynRolloutAdjointFbArgs& af, hipStream_t st)
{
  const RdynRolloutAdjointArgs& a = af.ax.a;
  const RdynExtArgs& x = af.ax.x;
  if (a.n_samples <= 0) return hipSuccess;
  if (a.integrator != RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER && a.integrator != RDYN_INTEGRATOR_RK4) return hipErrorInvalidValue;
  if (a.t.n_comps < 0 || a.t.n_comps > RDYN_MAX_COMPONENTS || a.n_steps < 0 || (a.n_steps > 0 && !a.tau) ||
      (a.n_steps > 1 && (!a.q_traj || !a.dq_traj)))
    return hipErrorInvalidValue;
  if (x.w ? (x.one < 0 || x.one > n_joints + 1 || x.step < 0 || af.ax.gw_step < 0) : af.ax.gw != nullptr) return hipErrorInvalidValue;
  if (!af.f.q_ref || !af.f.kp || af.f.ref_step < 0 || (af.f.hold | af.f.per_sample) & ~1) return hipErrorInvalidValue;
  if (af.g.gref_step < 0 || af.g.gu_step < 0 || af.g.accumulate & ~1) return hipErrorInvalidValue;
  const bool rk4 = a.integrator == RDYN_INTEGRATOR_RK4;
  if (x.w) return rk4 ? rdyn_launch_rollout_adjoint_feedback_ext_rk4(n_joints, af, st) : rdyn_launch_rollout_adjoint_feedback_ext_euler(n_joints, af, st);
  return rk4 ? rdyn_launch_rollout_adjoint_feedback_rk4(n_joints, af, st) : rdyn_launch_rollout_adjoint_feedback_euler(n_joints, af, st);
}
#endif
