// rdyn_fwd_dyn_comp.hip -- forward dynamics with friction and spring components (rdyn_forward_dynamics_components):
//     ddq = FD(q, dq, tau - tau_c(q, dq)),
// tau_c the component torque rdyn_components_regressor accumulates into a zero-initialised tau_add (rdyn_component_row.h).
//   k_fwd_dyn_comp<NJ>   k_fwd_dyn's text (rdyn_fwd_dyn_kernel.inc) with the subtraction between the torque loads and the evaluation; the
//     component table travels in the kernel arguments, as in k_components.  A translation unit of its own: it builds beside
//     rdyn_fwd_dyn.hip, whose code objects stay what they were.
// The chunked route's variant of the solve kernel is in rdyn_fwd_dyn.hip.
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_record_stage.h"
#include "rdyn_fwd_dyn_body.h"
#include "rdyn_component_row.h"
#include "rdyn_launch_util.h"

namespace
{
template <int NJ>
__global__ __launch_bounds__(64) void k_fwd_dyn_comp(const RdynFwdDynCompArgs ac)
{
  const RdynFwdDynArgs& a = ac.f;
  // by chain joint f, a run-time loop over the list inside: list order per joint, and rhs is never indexed dynamically
#define RDYN_FWD_KERNEL_RHS(rhs)                                                                         \
  _Pragma("unroll") for (int f = 0; f < NJ; ++f)                                                         \
  {                                                                                                      \
    const int idx = c->j[f].in_idx;                                                                      \
    if (idx >= 0) rhs[f] -= joint_component_torque(ac.t, idx, qp[idx * a.in_sj], dqp[idx * a.in_sj]);    \
  }
#define RDYN_FWD_LINK_WRENCH(f, R, t, fo, no)
#include "rdyn_fwd_dyn_kernel.inc"
#undef RDYN_FWD_LINK_WRENCH
#undef RDYN_FWD_KERNEL_RHS
}

template <int NJ>
hipError_t launch_fwd_comp_nj(const RdynFwdDynCompArgs& a, hipStream_t st)
{
  const size_t lds = a.f.staged ? (size_t)64 * (size_t)(a.f.staged | 1) * 8 : 0;
  hipLaunchKernelGGL((k_fwd_dyn_comp<NJ>), dim3((unsigned)((a.f.n_samples + 63) / 64)), dim3(64), lds, st, a);
  return hipGetLastError();
}
}  // namespace

hipError_t rdyn_launch_forward_dynamics_components(int n_joints, const RdynFwdDynCompArgs& a, hipStream_t st)
{
  if (a.f.n_samples <= 0) return hipSuccess;
  if (a.t.n_comps < 0 || a.t.n_comps > RDYN_MAX_COMPONENTS) return hipErrorInvalidValue;
#define CALL(N) launch_fwd_comp_nj<N>(a, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}
