// rdyn_fwd_dyn_ext.hip -- forward dynamics with external link wrenches (rdyn_forward_dynamics_ext):
//     ddq = FD(q, dq, tau - tau_c(q, dq) - tau_E(q, ext)),
// tau_E the joint torque of the wrenches alone in the convention of rdyn_joint_torque_ext (rdyn_ext_wrench.h).
//   k_fwd_dyn_ext<NJ>   k_fwd_dyn's text (rdyn_fwd_dyn_kernel.inc) with the component subtraction of k_fwd_dyn_comp in front of the
//     evaluation and the link-wrench hook of rdyn_fwd_dyn_body.inc filled: still ONE launch, the wrench read where its link is swept
//     (every link: 6 doubles per link; one link: 6 doubles per lane, loaded with the torques).  A translation unit of its own: it builds
//     beside rdyn_fwd_dyn.hip and rdyn_fwd_dyn_comp.hip, whose code objects stay what they were.
// The chunked route needs no kernel of its own: the wrench recursion that writes h into the chunk image (rdyn_long_kin.hip) takes the
// wrenches and writes h + tau_E.
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_record_stage.h"
#include "rdyn_fwd_dyn_body.h"
#include "rdyn_component_row.h"
#include "rdyn_ext_wrench.h"
#include "rdyn_launch_util.h"

namespace
{
template <int NJ>
__global__ __launch_bounds__(64) void k_fwd_dyn_ext(const RdynFwdDynExtArgs ax)
{
  const RdynFwdDynArgs& a = ax.c.f;
  // the components as in k_fwd_dyn_comp; then the sample's wrenches: s is the lane's sample
#define RDYN_FWD_KERNEL_RHS(rhs)                                                                           \
  _Pragma("unroll") for (int f = 0; f < NJ; ++f)                                                           \
  {                                                                                                        \
    const int idx = c->j[f].in_idx;                                                                        \
    if (idx >= 0) rhs[f] -= joint_component_torque(ax.c.t, idx, qp[idx * a.in_sj], dqp[idx * a.in_sj]);    \
  }                                                                                                        \
  ExtEval xe;                                                                                              \
  xe.rec = ax.x.w + s * ax.x.ss;                                                                           \
  xe.se = ax.x.se;                                                                                         \
  xe.one = ax.x.one;                                                                                       \
  xe.l = xe.a = mk(0, 0, 0);                                                                               \
  if (xe.one) ext_load6(xe.rec, xe.se, xe.l, xe.a);                                                        \
  V3 pl = mk(0, 0, 0);
#define RDYN_FWD_LINK_WRENCH(f, R, t, fo, no) ext_link_wrench(xe, f + 1, R, t, pl, fo, no);
#include "rdyn_fwd_dyn_kernel.inc"
#undef RDYN_FWD_LINK_WRENCH
#undef RDYN_FWD_KERNEL_RHS
}

template <int NJ>
hipError_t launch_fwd_ext_nj(const RdynFwdDynExtArgs& a, hipStream_t st)
{
  const size_t lds = a.c.f.staged ? (size_t)64 * (size_t)(a.c.f.staged | 1) * 8 : 0;
  hipLaunchKernelGGL((k_fwd_dyn_ext<NJ>), dim3((unsigned)((a.c.f.n_samples + 63) / 64)), dim3(64), lds, st, a);
  return hipGetLastError();
}
}  // namespace

hipError_t rdyn_launch_forward_dynamics_ext(int n_joints, const RdynFwdDynExtArgs& a, hipStream_t st)
{
  if (a.c.f.n_samples <= 0) return hipSuccess;
  if (a.c.t.n_comps < 0 || a.c.t.n_comps > RDYN_MAX_COMPONENTS) return hipErrorInvalidValue;
  if (!a.x.w || a.x.one < 0 || a.x.one > n_joints + 1) return hipErrorInvalidValue;
#define CALL(N) launch_fwd_ext_nj<N>(a, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}
