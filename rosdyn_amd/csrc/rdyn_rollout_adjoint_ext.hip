// rdyn_rollout_adjoint_ext.hip -- the adjoint of a batched rollout with external link wrenches (rdyn_rollout_adjoint_ext; no counterpart
// in the reference): the exact transpose of the scheme k_rollout_ext integrates.  k_rollout_adjoint_ext<NJ, INTEGRATOR> IS
// k_rollout_adjoint (rdyn_rollout_adjoint_body.inc, RDYN_ADJ_EXT on) with vjp replaced by the product of
// rdyn_forward_dynamics_vjp_ext: evaluated with the wrench of step t, held over the step and taken at each stage's own q; the RK4 stage
// states are rebuilt with FD_E (fwd_dyn_eval_ext).  Still ONE launch for the horizon, one lane per sample.
//   the wrenches   one link: 6 doubles per lane, loaded with the step's torques.  Every link: nothing is carried, each evaluation and
//                  each KIND 0 column reads a link's doubles where it sweeps the link (k_rollout_ext's choice, for the same registers).
//   gw             every product adds -(d tau_E / d ext)' w, 6 doubles per link, to the lane's OWN record of the step in memory, zeroed
//                  when the step begins: with RK4 the sum of the four stage products, last stage first.  gw_step = 0: one record, zeroed
//                  once, the sum over the steps in the order of the backward sweep.  No lane touches another's record and no atomics:
//                  the same bits every run, and with a step stride the same bits however the horizon is split into chained calls.
// A sample that fails at a backward step gets NaN in that step's record and every earlier one (gw_step = 0: in the whole record).
// Compiled once per integrator (RDYN_ADJ_EXT_INTEGRATOR) so that the two halves build in parallel.
#include <hip/hip_runtime.h>
#include "rdyn_rollout_adjoint_body.h"
#include "rdyn_ext_wrench.h"
#include "rdyn_launch_util.h"

#ifndef RDYN_ADJ_EXT_INTEGRATOR
#error "RDYN_ADJ_EXT_INTEGRATOR selects the integrator this object holds"
#endif

namespace
{
template <int NJ, int INTEGRATOR>
__global__ __launch_bounds__(64) void k_rollout_adjoint_ext(const RdynRolloutAdjointExtArgs ax)
{
  const RdynRolloutAdjointArgs& a = ax.a;
#define RDYN_ADJ_PARAMS 0
#define RDYN_ADJ_EXT 1
#include "rdyn_rollout_adjoint_body.inc"
#undef RDYN_ADJ_EXT
#undef RDYN_ADJ_PARAMS
}

template <int NJ>
hipError_t launch_adjoint_ext_nj(const RdynRolloutAdjointExtArgs& a, hipStream_t st)
{
  const size_t lds = a.a.staged ? (size_t)64 * (size_t)(a.a.n_active | 1) * 8 : 0;
  hipLaunchKernelGGL((k_rollout_adjoint_ext<NJ, RDYN_ADJ_EXT_INTEGRATOR>), dim3((unsigned)((a.a.n_samples + 63) / 64)), dim3(64), lds, st, a);
  return hipGetLastError();
}
}  // namespace

// (the preprocessor does not see the enumerators: the build hands over their values)
static_assert(RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER == 0 && RDYN_INTEGRATOR_RK4 == 1, "the Makefile names the integrators by these values");
#if RDYN_ADJ_EXT_INTEGRATOR == 1
#define RDYN_ADJ_EXT_LAUNCH rdyn_launch_rollout_adjoint_ext_rk4
#elif RDYN_ADJ_EXT_INTEGRATOR == 0
#define RDYN_ADJ_EXT_LAUNCH rdyn_launch_rollout_adjoint_ext_euler
#else
#error "RDYN_ADJ_EXT_INTEGRATOR is 0 (semi-implicit Euler) or 1 (RK4)"
#endif

hipError_t RDYN_ADJ_EXT_LAUNCH(int n_joints, const RdynRolloutAdjointExtArgs& ax, hipStream_t st)
{
  const RdynRolloutAdjointArgs& a = ax.a;
  if (a.n_samples <= 0) return hipSuccess;
  if (a.integrator != RDYN_ADJ_EXT_INTEGRATOR) return hipErrorInvalidValue;
  if (a.t.n_comps < 0 || a.t.n_comps > RDYN_MAX_COMPONENTS || a.n_steps < 0 || (a.n_steps > 0 && !a.tau) ||
      (a.n_steps > 1 && (!a.q_traj || !a.dq_traj)))
    return hipErrorInvalidValue;
  if (!ax.x.w || ax.x.one < 0 || ax.x.one > n_joints + 1 || ax.x.step < 0 || ax.gw_step < 0) return hipErrorInvalidValue;
#define CALL(N) launch_adjoint_ext_nj<N>(ax, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}
