// rdyn_rollout_adjoint_fb_params.hip -- the adjoint of a closed-loop rollout with the gradients with respect to the model's parameters
// (rdyn_rollout_adjoint_feedback_parameters; no counterpart in the reference).  k_rollout_adjoint_fb_params<NJ, INTEGRATOR> IS
// k_rollout_adjoint (rdyn_rollout_adjoint_body.inc) with RDYN_ADJ_FB and RDYN_ADJ_PARAMS both on and no wrenches: the backward sweep of
// k_rollout_adjoint_fb -- the same bits in gq0, gdq0, gtau, the status and the law's gradients -- and beside it every product adds
//     -Y(X, ddq)' w   and   -C(X)' w,   w = M^-1 seed,
// to the lane's own element-major accumulators, as k_rollout_adjoint_params does (rdyn_rollout_adjoint_params.hip has the accumulators,
// the status array and the fixed-order reduction).  The product is taken at the command the forward call applied there: the held command
// of the step (hold = 1, semi-implicit Euler) or the command formed at the stage state (hold = 0 with RK4), rebuilt by fb_command before
// the product.  The rows are added BEFORE fb_transpose replaces the product's tau_bar by the gradient with respect to the feed-forward
// torque: they see w = M^-1 seed.  The law does not depend on the model, so there is no further term.
// A sample that fails anywhere on the horizon contributes nothing to the sums (its status in the workspace is -1) and is NaN in its own
// rows of the state and law gradients, as in the two sibling kernels.
// Compiled once per integrator (RDYN_ADJ_FB_PARAMS_INTEGRATOR) so that the two halves build in parallel.
#include <hip/hip_runtime.h>
#include "rdyn_rollout_adjoint_body.h"
#include "rdyn_feedback_law.h"
#include "rdyn_feedback_transpose.h"
#include "rdyn_launch_util.h"

#ifndef RDYN_ADJ_FB_PARAMS_INTEGRATOR
#error "RDYN_ADJ_FB_PARAMS_INTEGRATOR selects the integrator this object holds"
#endif

namespace
{
template <int NJ, int INTEGRATOR>
__global__ __launch_bounds__(64) void k_rollout_adjoint_fb_params(const RdynRolloutAdjointFbArgs af, const RdynAdjointParamAcc p)
{
  const RdynRolloutAdjointArgs& a = af.ax.a;
  const RdynFeedbackArgs& fb = af.f;
  const RdynFeedbackGradArgs& gf = af.g;
#define RDYN_ADJ_PARAMS 1
#define RDYN_ADJ_EXT 0
#define RDYN_ADJ_FB 1
#include "rdyn_rollout_adjoint_body.inc"
#undef RDYN_ADJ_FB
#undef RDYN_ADJ_EXT
#undef RDYN_ADJ_PARAMS
}

template <int NJ>
hipError_t launch_adjoint_fb_params_nj(const RdynRolloutAdjointFbArgs& a, const RdynAdjointParamAcc& p, hipStream_t st)
{
  const RdynRolloutAdjointArgs& r = a.ax.a;
  const size_t lds = (r.staged || a.g.staged) ? (size_t)64 * (size_t)(r.n_active | 1) * 8 : 0;
  hipLaunchKernelGGL((k_rollout_adjoint_fb_params<NJ, RDYN_ADJ_FB_PARAMS_INTEGRATOR>), dim3((unsigned)((r.n_samples + 63) / 64)), dim3(64), lds, st,
                     a, p);
  return hipGetLastError();
}
}  // namespace

// (the preprocessor does not see the enumerators: the build hands over their values)
static_assert(RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER == 0 && RDYN_INTEGRATOR_RK4 == 1, "the Makefile names the integrators by these values");
#if RDYN_ADJ_FB_PARAMS_INTEGRATOR == 1
#define RDYN_ADJ_FB_PARAMS_LAUNCH rdyn_launch_rollout_adjoint_feedback_params_rk4
#elif RDYN_ADJ_FB_PARAMS_INTEGRATOR == 0
#define RDYN_ADJ_FB_PARAMS_LAUNCH rdyn_launch_rollout_adjoint_feedback_params_euler
#else
#error "RDYN_ADJ_FB_PARAMS_INTEGRATOR is 0 (semi-implicit Euler) or 1 (RK4)"
#endif

hipError_t RDYN_ADJ_FB_PARAMS_LAUNCH(int n_joints, const RdynRolloutAdjointFbArgs& af, double* acc, int64_t ld, int32_t* status, int n_comp_cols,
                                     hipStream_t st)
{
  const RdynRolloutAdjointArgs& a = af.ax.a;
  if (a.n_samples <= 0) return hipSuccess;
  if (a.integrator != RDYN_ADJ_FB_PARAMS_INTEGRATOR || !acc || !status || ld < a.n_samples || n_comp_cols < 0 ||
      n_comp_cols > 3 * RDYN_MAX_COMPONENTS)
    return hipErrorInvalidValue;
  if (a.t.n_comps < 0 || a.t.n_comps > RDYN_MAX_COMPONENTS || a.n_steps < 0 || (a.n_steps > 0 && !a.tau) ||
      (a.n_steps > 1 && (!a.q_traj || !a.dq_traj)))
    return hipErrorInvalidValue;
  if (af.ax.x.w || af.ax.gw) return hipErrorInvalidValue;  // the wrench path has no parameter rows yet
  if (!af.f.q_ref || !af.f.kp || af.f.ref_step < 0 || (af.f.hold | af.f.per_sample) & ~1) return hipErrorInvalidValue;
  if (af.g.gref_step < 0 || af.g.gu_step < 0 || af.g.accumulate & ~1) return hipErrorInvalidValue;
  RdynAdjointParamAcc p;
  p.acc = acc;
  p.ld = ld;
  p.status = status;
  p.n_comp_cols = n_comp_cols;
#define CALL(N) launch_adjoint_fb_params_nj<N>(af, p, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}
