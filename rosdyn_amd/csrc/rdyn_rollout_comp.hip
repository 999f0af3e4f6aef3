// rdyn_rollout_comp.hip -- rollouts with friction and spring components (rdyn_rollout_components): T steps of
//     x' = (dq, FD(q, dq, tau_t - tau_c(q, dq))),
// tau_c evaluated at every integrator stage at that stage's own state (RK4: the stage state and the stage velocity).
//   k_rollout_comp<NJ, INTEGRATOR>   k_rollout's text (rdyn_rollout_body.inc) with the subtraction immediately before each evaluation; the
//     component table travels in the kernel arguments, as in k_components.  The loop over the table has a run-time trip count and a
//     wave-uniform index, so like the chain constants (per_evaluation, rdyn_rollout_body.h) its entries are read by scalar loads at every
//     evaluation and nothing derived from them is carried in vector registers across one.  A translation unit of its own: it builds
//     beside rdyn_rollout.hip, whose code objects stay what they were.
// The chunked route (more than RDYN_MAX_SWEPT_JOINTS input joints) hands the stage state to the solve kernel's variant (rdyn_fwd_dyn.hip).
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_record_stage.h"
#include "rdyn_fwd_dyn_body.h"
#include "rdyn_rollout_body.h"
#include "rdyn_component_row.h"
#include "rdyn_launch_util.h"

namespace
{
template <int NJ, int INTEGRATOR>
__global__ __launch_bounds__(64) void k_rollout_comp(const RdynRolloutCompArgs ac)
{
  const RdynRolloutArgs& a = ac.r;
  // by chain joint f, a run-time loop over the list inside: list order per joint, and the state is never indexed dynamically
#define RDYN_ROLLOUT_RHS(q, dq, rhs)                                                   \
  _Pragma("unroll") for (int f = 0; f < NJ; ++f)                                       \
  {                                                                                    \
    const int idx = c->j[f].in_idx;                                                    \
    if (idx >= 0) rhs[f] -= joint_component_torque(ac.t, idx, q[f], dq[f]);            \
  }
#define RDYN_ROLLOUT_TAKE
#define RDYN_ROLLOUT_PREFETCH
#define RDYN_ROLLOUT_EVAL(c, q, dq, rhs) fwd_dyn_eval<NJ>(c, q, dq, rhs)
#include "rdyn_rollout_body.inc"
#undef RDYN_ROLLOUT_EVAL
#undef RDYN_ROLLOUT_PREFETCH
#undef RDYN_ROLLOUT_TAKE
#undef RDYN_ROLLOUT_RHS
}

template <int NJ>
hipError_t launch_rollout_comp_nj(const RdynRolloutCompArgs& a, hipStream_t st)
{
  const size_t lds = a.r.staged ? (size_t)64 * (size_t)(a.r.n_active | 1) * 8 : 0;
  const dim3 grid((unsigned)((a.r.n_samples + 63) / 64));
  if (a.r.integrator == RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER)
    hipLaunchKernelGGL((k_rollout_comp<NJ, RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER>), grid, dim3(64), lds, st, a);
  else
    hipLaunchKernelGGL((k_rollout_comp<NJ, RDYN_INTEGRATOR_RK4>), grid, dim3(64), lds, st, a);
  return hipGetLastError();
}
}  // namespace

hipError_t rdyn_launch_rollout_components(int n_joints, const RdynRolloutCompArgs& a, hipStream_t st)
{
  if (a.r.n_samples <= 0) return hipSuccess;
  if (a.r.integrator != RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER && a.r.integrator != RDYN_INTEGRATOR_RK4) return hipErrorInvalidValue;
  if (a.t.n_comps < 0 || a.t.n_comps > RDYN_MAX_COMPONENTS) return hipErrorInvalidValue;
#define CALL(N) launch_rollout_comp_nj<N>(a, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}
