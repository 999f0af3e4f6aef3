// rdyn_rollout_ext.hip -- rollouts with external link wrenches (rdyn_rollout_ext): T steps of
//     x' = (dq, FD(q, dq, tau_t - tau_c(q, dq) - tau_E(q, ext_t))),
// the wrench of step t held over the step like tau_t and evaluated at every integrator stage at that stage's own q (tau_E depends on q:
// this is what a caller cannot fold into tau).
//   k_rollout_ext<NJ, INTEGRATOR>   k_rollout's text (rdyn_rollout_body.inc) with the component subtraction of k_rollout_comp and the
//     evaluation of rdyn_ext_wrench.h: still ONE launch for the horizon.
//       one link    6 doubles per lane, in registers.  With a per-step sequence they are handled like the torques: the evaluation takes
//                   its copy, and the wrench of step t + 1 is requested into the same registers where the torques of step t + 1 are, to
//                   arrive while the last evaluation of step t runs.  A constant wrench is read once.
//       every link  6 (NJ + 1) doubles per lane: these kernels sit at one wave per SIMD with their accumulation registers in use, so
//                   nothing is carried: each evaluation reads a link's six doubles where it sweeps the link (L2 serves the re-reads of
//                   RK4's four stages).
//     A translation unit of its own: it builds beside rdyn_rollout.hip and rdyn_rollout_comp.hip, whose code objects stay what they were.
// The chunked route hands the step's wrenches to the wrench recursion of each stage's pass (rdyn_api_dynamics.cpp).
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_record_stage.h"
#include "rdyn_fwd_dyn_body.h"
#include "rdyn_rollout_body.h"
#include "rdyn_component_row.h"
#include "rdyn_ext_wrench.h"
#include "rdyn_launch_util.h"

namespace
{
template <int NJ, int INTEGRATOR>
__global__ __launch_bounds__(64) void k_rollout_ext(const RdynRolloutExtArgs ax)
{
  const RdynRolloutArgs& a = ax.c.r;
  const RdynExtArgs& x = ax.x;
  // the lane's record of step 0 (lanes past the batch leave at the head of the body and read nothing)
  const int64_t s_ext = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool in_batch = s_ext < a.n_samples;
  const double* const xp = x.w + (in_batch ? s_ext : 0) * x.ss;
  ExtEval xe;
  xe.rec = xp;
  xe.se = x.se;
  xe.one = x.one;
  xe.l = xe.a = mk(0, 0, 0);
  V3 wl = mk(0, 0, 0), wa = mk(0, 0, 0);  // one link: the wrench of the step (of the next one once the evaluation has its copy)
  if (x.one && in_batch && a.n_steps > 0) ext_load6(xp, x.se, wl, wa);
#define RDYN_ROLLOUT_RHS(q, dq, rhs)                                                   \
  _Pragma("unroll") for (int f = 0; f < NJ; ++f)                                       \
  {                                                                                    \
    const int idx = c->j[f].in_idx;                                                    \
    if (idx >= 0) rhs[f] -= joint_component_torque(ax.c.t, idx, q[f], dq[f]);          \
  }
#define RDYN_ROLLOUT_TAKE                            \
  if (x.one)                                         \
  {                                                  \
    xe.l = wl;                                       \
    xe.a = wa;                                       \
  }                                                  \
  else                                               \
    xe.rec = xp + (int64_t)t * x.step;
#define RDYN_ROLLOUT_PREFETCH \
  if (x.one && x.step != 0) ext_load6(xp + (int64_t)(t + 1) * x.step, x.se, wl, wa);
#define RDYN_ROLLOUT_EVAL(c, q, dq, rhs) fwd_dyn_eval_ext<NJ>(c, q, dq, rhs, xe)
#include "rdyn_rollout_body.inc"
#undef RDYN_ROLLOUT_EVAL
#undef RDYN_ROLLOUT_PREFETCH
#undef RDYN_ROLLOUT_TAKE
#undef RDYN_ROLLOUT_RHS
}

template <int NJ>
hipError_t launch_rollout_ext_nj(const RdynRolloutExtArgs& a, hipStream_t st)
{
  const RdynRolloutArgs& r = a.c.r;
  const size_t lds = r.staged ? (size_t)64 * (size_t)(r.n_active | 1) * 8 : 0;
  const dim3 grid((unsigned)((r.n_samples + 63) / 64));
  if (r.integrator == RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER)
    hipLaunchKernelGGL((k_rollout_ext<NJ, RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER>), grid, dim3(64), lds, st, a);
  else
    hipLaunchKernelGGL((k_rollout_ext<NJ, RDYN_INTEGRATOR_RK4>), grid, dim3(64), lds, st, a);
  return hipGetLastError();
}
}  // namespace

hipError_t rdyn_launch_rollout_ext(int n_joints, const RdynRolloutExtArgs& a, hipStream_t st)
{
  const RdynRolloutArgs& r = a.c.r;
  if (r.n_samples <= 0) return hipSuccess;
  if (r.integrator != RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER && r.integrator != RDYN_INTEGRATOR_RK4) return hipErrorInvalidValue;
  if (a.c.t.n_comps < 0 || a.c.t.n_comps > RDYN_MAX_COMPONENTS) return hipErrorInvalidValue;
  if (!a.x.w || a.x.one < 0 || a.x.one > n_joints + 1 || a.x.step < 0) return hipErrorInvalidValue;
#define CALL(N) launch_rollout_ext_nj<N>(a, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}
