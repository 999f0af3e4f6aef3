// rdyn_rollout_adjoint.hip -- the adjoint of a batched rollout (rdyn_rollout_adjoint; no counterpart in the reference): the exact
// transpose of the discrete scheme k_rollout / k_rollout_comp integrate, backwards over the horizon from the seeds on the end state (and,
// optionally, on every trajectory record) to the gradients with respect to the initial state and every step's torques.
//
//   lambda_T = g_end + g_traj[T - 1];   for t = T - 1 .. 0:   (lambda_t, gtau_t) = step'(x_t, tau_t; lambda_{t + 1}),   t >= 1: lambda_t += g_traj[t - 1]
//
// x_0 is the batch's state, x_t record t - 1 of the forward call's trajectory (traj_every = 1).  With vjp(q, v, tau; a_bar) -> (q_bar,
// v_bar, tau_bar) the product of rdyn_fwd_dyn_vjp_body.h, the step transposes are
//   semi-implicit Euler (v' = v + dt a, q' = q + dt v'):   lv* = lv' + dt lq',   mu = dt lv*,   (q_bar, v_bar, tau_bar) = vjp(x_t, tau_t; mu),
//     lq = lq' + q_bar,   lv = lv* + v_bar,   gtau_t = tau_bar
//   RK4: the stage states X1 .. X4 are rebuilt from x_t as rdyn_rollout_body.inc builds them (three plain evaluations); with
//     b = 1/6, 1/3, 1/3, 1/6 and c = ., dt/2, dt/2, dt:   kq_i = dt b_i lq' + carry_q,   kv_i likewise,   for i = 4 .. 1:
//     (q_bar, v_bar, tau_bar) = vjp(X_i, tau_t; kv_i),   X_bar_i = (q_bar, kq_i + v_bar),   gtau_t += tau_bar,   x_bar += X_bar_i,
//     carry = c_i X_bar_i (into stage i - 1);   lambda_t = x_bar, which started as lambda'.
// Component torques and their slopes are taken at each stage's own state, as in the forward call.
//
//   k_rollout_adjoint<NJ, INTEGRATOR>   chains the unrolled kernels sweep: ONE launch for the horizon, one lane per sample.  lambda stays in
//     registers between the steps; backward step t reads x_t, tau_t and the running seeds that are due (3 n .. 5 n doubles) and writes
//     gtau_t (or adds it to the running sum that leaves once, gtau_step = 0).  The step loop has a run-time trip count and ONE body: a
//     horizon split anywhere into chained calls gives the same bits.  RK4's stages are run-time loops too, one copy of each evaluation in
//     the code object; the three rebuilt stage states (6 NJ doubles) are KEPT across the four products -- recomputing stage i costs i - 1
//     plain evaluations, six per step on top of the three, against registers that the 9- and 10-joint kernels spill either way
//     (DESIGN.md section 3 has the compiler's figures).
//   k_adjoint_update   more than RDYN_MAX_SWEPT_JOINTS input joints: CORRECT BUT NOT FAST.  The host loops over steps and stages on the
//     stream (rdyn_api_dynamics.cpp): the chunked rdyn_forward_dynamics_vjp route for every product, the chunked forward dynamics for the RK4
//     stage rebuild, and this element-wise kernel for everything between them.  State, stage and seed buffers are in the caller's
//     workspace in the batch's layout: one thread per double, every access contiguous.
// A sample with a failed pivot or a non-finite value in any evaluation gets status -1 and, from that backward step on, quiet NaN in every
// output (explicitly: the flag is sticky).  The trajectory of a sample whose forward rollout failed holds NaN records, so it fails here.
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_record_stage.h"
#include "rdyn_fwd_dyn_body.h"
#include "rdyn_rollout_body.h"
#include "rdyn_component_row.h"
#include "rdyn_fwd_dyn_vjp_body.h"
#include "rdyn_rollout_adjoint_body.h"
#include "rdyn_launch_util.h"

namespace
{
template <int NJ, int INTEGRATOR>
__global__ __launch_bounds__(64) void k_rollout_adjoint(const RdynRolloutAdjointArgs a)
{
#define RDYN_ADJ_PARAMS 0
#define RDYN_ADJ_EXT 0
#include "rdyn_rollout_adjoint_body.inc"
#undef RDYN_ADJ_EXT
#undef RDYN_ADJ_PARAMS
}

// thread e: double e of the (contiguous) arrays; its sample is e / n (sample-major) or e % n_samples (element-major)
__global__ __launch_bounds__(256) void k_adjoint_update(const RdynAdjointUpdateArgs a)
{
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.count) return;
  const int64_t s = a.element_major ? e % a.n_samples : e / a.n;
  const bool first = a.element_major ? e < a.n_samples : e == s * a.n;  // the sample's first double keeps its status
  const double qnan = __builtin_nan("");
  const double dt = a.dt;
  switch (a.op)
  {
  case RDYN_ADJ_OP_INIT:
  {
    double x = a.a ? a.a[e] : 0.0, v = a.c ? a.c[e] : 0.0;
    if (a.b) x += a.b[e];
    if (a.d) v += a.d[e];
    a.lq[e] = x;
    a.lv[e] = v;
    if (first) a.st_run[s] = 1;
    return;
  }
  case RDYN_ADJ_OP_EULER_PRE:
  {
    const double v = fma(dt, a.lq[e], a.lv[e]);
    a.lv[e] = v;
    a.mv[e] = dt * v;
    return;
  }
  case RDYN_ADJ_OP_EULER_POST:
  {
    const int32_t run = a.st_run[s];
    const int32_t st = a.st_stage[s] < run ? a.st_stage[s] : run;
    const bool alive = st > 0;
    const double g = alive ? a.tb[e] : qnan;
    a.lq[e] = alive ? a.lq[e] + a.qb[e] : qnan;
    a.lv[e] = alive ? a.lv[e] + a.vb[e] : qnan;
    if (a.gtau) a.gtau[e] = a.gtau_add ? a.gtau[e] + g : g;
    if (first) a.st_run[s] = st;
    return;
  }
  case RDYN_ADJ_OP_RK4_FWD:
  {
    // a = q, b = dq of x_t; c = the stage's velocity, d = the acceleration the pass returned
    a.sq[e] = fma(a.cdt, a.c[e], a.a[e]);
    a.sv[e] = fma(a.cdt, a.d[e], a.b[e]);
    return;
  }
  case RDYN_ADJ_OP_RK4_PRE:
  {
    a.xq[e] = a.lq[e];
    a.xv[e] = a.lv[e];
    a.kq[e] = 0.0;
    a.kv[e] = 0.0;
    if (a.gtau && !a.gtau_add) a.gtau[e] = 0.0;
    if (a.mq) a.mq[e] = 0.0;  // the step's gtau accumulates here when the caller's is a running sum
    return;
  }
  case RDYN_ADJ_OP_RK4_SEED:
  {
    const double dtb = dt * a.wgt;
    a.kq[e] = fma(dtb, a.lq[e], a.kq[e]);
    a.mv[e] = fma(dtb, a.lv[e], a.kv[e]);
    return;
  }
  case RDYN_ADJ_OP_RK4_POST:
  {
    const int32_t run = a.st_run[s];
    const int32_t st = a.st_stage[s] < run ? a.st_stage[s] : run;
    const double qb = a.qb[e], bv = a.kq[e] + a.vb[e];
    a.mq[e] += a.tb[e];
    a.xq[e] += qb;
    a.xv[e] += bv;
    a.kq[e] = a.cdt * qb;
    a.kv[e] = a.cdt * bv;
    if (first) a.st_run[s] = st;
    return;
  }
  case RDYN_ADJ_OP_RK4_END:
  {
    const bool alive = a.st_run[s] > 0;
    const double g = alive ? a.mq[e] : qnan;
    a.lq[e] = alive ? a.xq[e] : qnan;
    a.lv[e] = alive ? a.xv[e] : qnan;
    if (a.gtau) a.gtau[e] = a.gtau_add ? a.gtau[e] + g : g;
    return;
  }
  case RDYN_ADJ_OP_ADD_SEED:
  {
    if (a.a) a.lq[e] += a.a[e];
    if (a.b) a.lv[e] += a.b[e];
    return;
  }
  case RDYN_ADJ_OP_OUT:
  {
    if (a.out_q) a.out_q[e] = a.lq[e];
    if (a.out_v) a.out_v[e] = a.lv[e];
    if (first && a.status) a.status[s] = a.st_run[s];
    return;
  }
  case RDYN_ADJ_OP_ZERO:
  {
    if (a.gtau) a.gtau[e] = 0.0;
    return;
  }
  default: return;
  }
}

template <int NJ>
hipError_t launch_adjoint_nj(const RdynRolloutAdjointArgs& a, hipStream_t st)
{
  const size_t lds = a.staged ? (size_t)64 * (size_t)(a.n_active | 1) * 8 : 0;
  const dim3 grid((unsigned)((a.n_samples + 63) / 64));
  if (a.integrator == RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER)
    hipLaunchKernelGGL((k_rollout_adjoint<NJ, RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER>), grid, dim3(64), lds, st, a);
  else
    hipLaunchKernelGGL((k_rollout_adjoint<NJ, RDYN_INTEGRATOR_RK4>), grid, dim3(64), lds, st, a);
  return hipGetLastError();
}
}  // namespace

hipError_t rdyn_launch_rollout_adjoint(int n_joints, const RdynRolloutAdjointArgs& a, hipStream_t st)
{
  if (a.n_samples <= 0) return hipSuccess;
  if (a.integrator != RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER && a.integrator != RDYN_INTEGRATOR_RK4) return hipErrorInvalidValue;
  if (a.t.n_comps < 0 || a.t.n_comps > RDYN_MAX_COMPONENTS || a.n_steps < 0 || (a.n_steps > 0 && !a.tau) ||
      (a.n_steps > 1 && (!a.q_traj || !a.dq_traj)))
    return hipErrorInvalidValue;
#define CALL(N) launch_adjoint_nj<N>(a, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}

hipError_t rdyn_launch_adjoint_update(const RdynAdjointUpdateArgs& a, hipStream_t st)
{
  if (a.count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_adjoint_update, dim3((unsigned)((a.count + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}
