// rdyn_rollout_adjoint_params.hip -- the adjoint of a batched rollout with the gradients with respect to the model's parameters
// (rdyn_rollout_adjoint_parameters; no counterpart in the reference).  k_rollout_adjoint_params<NJ, INTEGRATOR> IS k_rollout_adjoint
// (rdyn_rollout_adjoint_body.inc, RDYN_ADJ_PARAMS on): the same backward sweep, the same bits in gq0, gdq0, gtau and the status; beside it
// every product -- one per step at the seed mu (semi-implicit Euler), four per step at the seeds kv_i (RK4) -- adds
//     -Y(X, ddq)' w  (ten entries per link, link_parameter_row)   and   -C(X)' w  (the component columns),   w = M^-1 seed,
// to the lane's OWN accumulators, element-major in the workspace: acc[col][sample], every access of a wave one contiguous run of 512
// bytes.  A lane whose sample fails anywhere on the horizon has accumulated whatever it has; its final verdict goes to a status array in
// the workspace and rdyn_launch_parameter_sums (rdyn_fwd_dyn_param_vjp.hip) leaves its column entries out: such a sample contributes
// nothing, not even from the steps before it failed.  That reduction has a fixed order, so gpi and gcomp are the same bits every run.
// Every NJ takes this route: the accumulators of 6 joints (60 columns, 30 KB per wave) would fit the LDS beside four waves per CU, those of
// 10 joints with components (56 KB) would not; one route keeps one text.
// Compiled once per integrator (RDYN_ADJ_PARAMS_INTEGRATOR) so that the two halves build in parallel.
#include <hip/hip_runtime.h>
#include "rdyn_rollout_adjoint_body.h"
#include "rdyn_launch_util.h"

#ifndef RDYN_ADJ_PARAMS_INTEGRATOR
#error "RDYN_ADJ_PARAMS_INTEGRATOR selects the integrator this object holds"
#endif

namespace
{
template <int NJ, int INTEGRATOR>
__global__ __launch_bounds__(64) void k_rollout_adjoint_params(const RdynRolloutAdjointArgs a, const RdynAdjointParamAcc p)
{
#define RDYN_ADJ_PARAMS 1
#define RDYN_ADJ_EXT 0
#include "rdyn_rollout_adjoint_body.inc"
#undef RDYN_ADJ_EXT
#undef RDYN_ADJ_PARAMS
}

template <int NJ>
hipError_t launch_adjoint_params_nj(const RdynRolloutAdjointArgs& a, const RdynAdjointParamAcc& p, hipStream_t st)
{
  const size_t lds = a.staged ? (size_t)64 * (size_t)(a.n_active | 1) * 8 : 0;
  hipLaunchKernelGGL((k_rollout_adjoint_params<NJ, RDYN_ADJ_PARAMS_INTEGRATOR>), dim3((unsigned)((a.n_samples + 63) / 64)), dim3(64), lds, st, a, p);
  return hipGetLastError();
}
}  // namespace

// (the preprocessor does not see the enumerators: the build hands over their values)
static_assert(RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER == 0 && RDYN_INTEGRATOR_RK4 == 1, "the Makefile names the integrators by these values");
#if RDYN_ADJ_PARAMS_INTEGRATOR == 1
#define RDYN_ADJ_PARAMS_LAUNCH rdyn_launch_rollout_adjoint_params_rk4
#elif RDYN_ADJ_PARAMS_INTEGRATOR == 0
#define RDYN_ADJ_PARAMS_LAUNCH rdyn_launch_rollout_adjoint_params_euler
#else
#error "RDYN_ADJ_PARAMS_INTEGRATOR is 0 (semi-implicit Euler) or 1 (RK4)"
#endif

hipError_t RDYN_ADJ_PARAMS_LAUNCH(int n_joints, const RdynRolloutAdjointArgs& a, double* acc, int64_t ld, int32_t* status, int n_comp_cols,
                                  hipStream_t st)
{
  if (a.n_samples <= 0) return hipSuccess;
  if (a.integrator != RDYN_ADJ_PARAMS_INTEGRATOR || !acc || !status || ld < a.n_samples || n_comp_cols < 0 ||
      n_comp_cols > 3 * RDYN_MAX_COMPONENTS)
    return hipErrorInvalidValue;
  if (a.t.n_comps < 0 || a.t.n_comps > RDYN_MAX_COMPONENTS || a.n_steps < 0 || (a.n_steps > 0 && !a.tau) ||
      (a.n_steps > 1 && (!a.q_traj || !a.dq_traj)))
    return hipErrorInvalidValue;
  RdynAdjointParamAcc p;
  p.acc = acc;
  p.ld = ld;
  p.status = status;
  p.n_comp_cols = n_comp_cols;
#define CALL(N) launch_adjoint_params_nj<N>(a, p, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}
