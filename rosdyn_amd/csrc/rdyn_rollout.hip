// rdyn_rollout.hip -- batched rollouts: T steps of x' = (dq, FD(q, dq, tau_t)) from (q0, dq0) under a torque sequence held over each step
// (rdyn_rollout; no counterpart in the reference, which has no integrator).  FD is rdyn_forward_dynamics' function of the chain as
// configured; the integrators are semi-implicit Euler (dq += dt ddq, then q += dt dq) and the classical RK4.
//
//   k_rollout<NJ, INTEGRATOR>   chains the unrolled kernels sweep: ONE launch, one lane per sample.  q and dq stay in registers from the
//     first step to the last; a step reads the sample's n torques and writes nothing unless a trajectory record is due.  The evaluation is
//     rdyn_fwd_dyn_body.h's, the one k_fwd_dyn runs.  The step loop has a run-time trip count and ONE body (not unrolled): a horizon split
//     anywhere into chained calls gives the same bits.  RK4's four stages are a run-time loop too (one copy of the evaluation in the
//     code object): across an evaluation the lane holds q, dq, the two weighted sums, the stage velocity (the next stage's dq-slope) and
//     the step's torques, 6 NJ doubles on top of the evaluation's own registers; Euler holds q, dq and the torques, 3 NJ.
//     One wave per SIMD: nothing hides the latency of the torque loads, so the torques of step t + 1 are requested into the same
//     registers right after the last evaluation of step t has taken its copy, and arrive while that evaluation runs.
//     Sample-major records (trajectory records, the end state) leave through SmallRecords (rdyn_record_stage.h) in whole lines under
//     k_fwd_dyn's condition (the host found them line-aligned with natural strides, the wave is full); otherwise 8-byte stores.
//   k_rollout_stage   more than RDYN_MAX_SWEPT_JOINTS input joints: the host runs the chunked forward dynamics once per stage on the
//     stream (rdyn_api_dynamics.cpp); this element-wise kernel forms the next stage state, accumulates the weighted sums, at the last stage
//     advances the state, writes the trajectory record that is due and keeps the status as the running minimum.  State and stage buffers are
//     in the caller's workspace in the batch's layout, so one thread per double, every access contiguous.
//   k_rollout_copy    the same route: initial state -> workspace (status 1), workspace -> end state (status out).
// A sample whose evaluation fails the pivot rule of rdyn_forward_dynamics gets status -1 and quiet NaN in its state from that step on
// (explicitly: the flag is sticky, it does not rely on NaN propagating through M).
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_record_stage.h"
#include "rdyn_fwd_dyn_body.h"
#include "rdyn_rollout_body.h"
#include "rdyn_launch_util.h"

namespace
{
template <int NJ, int INTEGRATOR>
__global__ __launch_bounds__(64) void k_rollout(const RdynRolloutArgs a)
{
#define RDYN_ROLLOUT_RHS(q, dq, rhs)
#define RDYN_ROLLOUT_TAKE
#define RDYN_ROLLOUT_PREFETCH
#define RDYN_ROLLOUT_EVAL(c, q, dq, rhs) fwd_dyn_eval<NJ>(c, q, dq, rhs)
#include "rdyn_rollout_body.inc"
#undef RDYN_ROLLOUT_EVAL
#undef RDYN_ROLLOUT_PREFETCH
#undef RDYN_ROLLOUT_TAKE
#undef RDYN_ROLLOUT_RHS
}

// thread e: double e of the (contiguous) state arrays; its sample is e / n (sample-major) or e % n_samples (element-major)
__global__ __launch_bounds__(256) void k_rollout_stage(const RdynRolloutStageArgs a)
{
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.count) return;
  const int64_t s = a.element_major ? e % a.n_samples : e / a.n;
  const int32_t run_old = a.st_run[s];
  const int32_t st = a.st_stage[s] < run_old ? a.st_stage[s] : run_old;
  const bool first = a.element_major ? e < a.n_samples : e == s * a.n;  // the sample's first double keeps its status
  const double acc = a.ddq[e];
  if (a.integrator == RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER)
  {
    const double qnan = __builtin_nan("");
    double v = fma(a.dt, acc, a.dq[e]);
    double x = fma(a.dt, v, a.q[e]);
    if (st < 0) v = x = qnan;
    a.dq[e] = v;
    a.q[e] = x;
    if (a.q_rec) a.q_rec[e] = x;
    if (a.dq_rec) a.dq_rec[e] = v;
    if (first) a.st_run[s] = st;
    return;
  }
  // RK4 stage a.stage has been evaluated at (sq, sv) -- (q, dq) themselves at stage 0 -- and gave acc
  const int stage = a.stage;
  const double wgt = (stage == 0 || stage == 3) ? 1.0 / 6.0 : 1.0 / 3.0;
  const double kq = stage == 0 ? a.dq[e] : a.sv[e];
  const double aq = fma(wgt, kq, stage == 0 ? 0.0 : a.aq[e]);
  const double av = fma(wgt, acc, stage == 0 ? 0.0 : a.av[e]);
  if (stage < 3)
  {
    const double cdt = stage == 2 ? a.dt : 0.5 * a.dt;  // of the NEXT stage
    a.aq[e] = aq;
    a.av[e] = av;
    a.sq[e] = fma(cdt, kq, a.q[e]);
    a.sv[e] = fma(cdt, acc, a.dq[e]);
  }
  else
  {
    const double qnan = __builtin_nan("");
    double x = fma(a.dt, aq, a.q[e]);
    double v = fma(a.dt, av, a.dq[e]);
    if (st < 0) v = x = qnan;
    a.q[e] = x;
    a.dq[e] = v;
    if (a.q_rec) a.q_rec[e] = x;
    if (a.dq_rec) a.dq_rec[e] = v;
  }
  if (first) a.st_run[s] = st;
}

__global__ __launch_bounds__(256) void k_rollout_copy(const RdynRolloutCopyArgs a)
{
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < a.count)
  {
    if (a.q_dst) a.q_dst[e] = a.q_src[e];
    if (a.dq_dst) a.dq_dst[e] = a.dq_src[e];
  }
  if (e < a.n_samples && a.st_dst) a.st_dst[e] = a.st_src ? a.st_src[e] : 1;
}

template <int NJ>
hipError_t launch_rollout_nj(const RdynRolloutArgs& a, hipStream_t st)
{
  const size_t lds = a.staged ? (size_t)64 * (size_t)(a.n_active | 1) * 8 : 0;
  const dim3 grid((unsigned)((a.n_samples + 63) / 64));
  if (a.integrator == RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER)
    hipLaunchKernelGGL((k_rollout<NJ, RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER>), grid, dim3(64), lds, st, a);
  else
    hipLaunchKernelGGL((k_rollout<NJ, RDYN_INTEGRATOR_RK4>), grid, dim3(64), lds, st, a);
  return hipGetLastError();
}
}  // namespace

hipError_t rdyn_launch_rollout(int n_joints, const RdynRolloutArgs& a, hipStream_t st)
{
  if (a.n_samples <= 0) return hipSuccess;
  if (a.integrator != RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER && a.integrator != RDYN_INTEGRATOR_RK4) return hipErrorInvalidValue;
#define CALL(N) launch_rollout_nj<N>(a, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}

hipError_t rdyn_launch_rollout_stage(const RdynRolloutStageArgs& a, hipStream_t st)
{
  if (a.count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rollout_stage, dim3((unsigned)((a.count + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t rdyn_launch_rollout_copy(const RdynRolloutCopyArgs& a, hipStream_t st)
{
  const int64_t m = a.count > a.n_samples ? a.count : a.n_samples;
  if (m <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rollout_copy, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}
