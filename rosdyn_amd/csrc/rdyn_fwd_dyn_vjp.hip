// rdyn_fwd_dyn_vjp.hip -- batched reverse-mode products of the forward dynamics (rdyn_forward_dynamics_vjp; no counterpart in the
// reference): with ddq = FD_c(q, dq, tau) and a seed ddq_bar per sample
//     tau_bar = M^-1 ddq_bar,   q_bar = dddq_dq' ddq_bar,   dq_bar = dddq_dv' ddq_bar,
// the matrices exactly those of rdyn_forward_dynamics_derivatives (rdyn_fwd_dyn_deriv.hip) -- which are never formed here.
//
//   k_fwd_dyn_vjp<NJ>   1 .. RDYN_MAX_SWEPT_JOINTS chain joints, one lane per sample, ONE launch, nothing but the 4 n inputs and the (up to)
//     4 n outputs of a sample touches memory.  The evaluation is rdyn_fwd_dyn_vjp_body.h's: one pair of triangular solves (the derivative
//     kernel needs 2 n + n) with the factor still in registers, then the tangent columns of k_torque_deriv, each reduced against
//     w = M^-1 ddq_bar while its rows appear.  No LDS but the SmallRecords tile of sample-major outputs (64 (n | 1) doubles).
//   k_vjp_products      more input joints: CORRECT BUT NOT FAST.  The host runs the chunked rdyn_forward_dynamics_derivatives into
//     element-major matrices in the workspace (3 n n doubles per sample of the chunk) and this kernel forms the three transposed
//     products, one lane per sample, 512 contiguous bytes per wave and access.  The seeds are read from a copy k_vjp_seed_copy made in
//     the workspace before the chunk's first pass (tau_bar may alias them, and an output doubles as the ddq buffer of that pass).
// A sample whose factorisation failed the pivot rule, or with a non-finite state, torque or seed, gets status -1 and quiet NaN in every
// output.
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_record_stage.h"
#include "rdyn_rollout_body.h"
#include "rdyn_fwd_dyn_vjp_body.h"
#include "rdyn_launch_util.h"

namespace
{
template <int NJ>
__global__ __launch_bounds__(64) void k_fwd_dyn_vjp(const RdynFwdDynVjpArgs a)
{
  ChainPtr c = as_const(a.chain);
  const int lane = threadIdx.x;
  const int64_t s_wave = (int64_t)blockIdx.x * 64;
  const int64_t s = s_wave + lane;
  if (s >= a.n_samples) return;
  const bool stg = a.staged && a.n_samples - s_wave >= 64;  // wave-uniform: a full wave's records leave in whole lines

  const double* __restrict__ qp = a.q + s * a.in_ss;
  const double* __restrict__ dqp = a.dq + s * a.in_ss;
  double rhs[NJ], ab[NJ], qb[NJ], vb[NJ];
  {
    const double* __restrict__ tp = a.tau + s * a.in_ss;
    const double* sp = a.ddq_bar + s * a.in_ss;  // (may alias tau_bar: every entry is read before the first store)
#pragma unroll
    for (int f = 0; f < NJ; ++f)
    {
      const int idx = c->j[f].in_idx;
      rhs[f] = idx >= 0 ? tp[idx * a.in_sj] : 0.0;
      ab[f] = idx >= 0 ? sp[idx * a.in_sj] : 0.0;
    }
  }
  SmallRecords sm;
  if (stg)
  {
    extern __shared__ __attribute__((aligned(16))) char vjp_stage_lds[];
    sm.init(vjp_stage_lds, c->n_active, lane);
  }
  const double qnan = __builtin_nan("");
  const int64_t ow = s_wave * a.in_ss, oo = s * a.in_ss;
  const bool ok = fwd_dyn_vjp_eval<NJ>(
      c, a.t, [&](int, int idx) { return qp[idx * a.in_sj]; }, [&](int, int idx) { return dqp[idx * a.in_sj]; }, rhs, ab, qb, vb,
      a.q_bar != nullptr, a.dq_bar != nullptr, [&](bool good, double (&ddq)[NJ]) {
        if (a.status) a.status[s] = good ? 1 : -1;
        if (!a.ddq) return;  // wave-uniform
        double v[NJ];
#pragma unroll
        for (int f = 0; f < NJ; ++f) v[f] = good ? ddq[f] : qnan;
        put_record<NJ>(c, sm, stg, v, a.ddq + ow, a.ddq + oo, a.in_sj, lane);
      });
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    ab[f] = ok ? ab[f] : qnan;
    qb[f] = ok ? qb[f] : qnan;
    vb[f] = ok ? vb[f] : qnan;
  }
  if (a.tau_bar) put_record<NJ>(c, sm, stg, ab, a.tau_bar + ow, a.tau_bar + oo, a.in_sj, lane);
  if (a.q_bar) put_record<NJ>(c, sm, stg, qb, a.q_bar + ow, a.q_bar + oo, a.in_sj, lane);
  if (a.dq_bar) put_record<NJ>(c, sm, stg, vb, a.dq_bar + ow, a.dq_bar + oo, a.in_sj, lane);
}

// ---- more input joints than the unrolled kernel sweeps: out_k = sum_i X[i + n k] seed_i from the workspace matrices -----------------------
__global__ __launch_bounds__(64) void k_vjp_products(const RdynVjpProductArgs a)
{
  extern __shared__ __attribute__((aligned(16))) double vpr_lds[];  // [n][64]: the seed
  const int n = a.n;
  const int lane = threadIdx.x;
  const int64_t sl = (int64_t)blockIdx.x * 64 + lane;  // sample of the chunk
  if (sl >= a.n_samples) return;
  const int64_t ld = a.ld;
  double* const x = vpr_lds + lane;
  const double* const sp = a.ddq_bar + sl * a.seed_ss;
  const double* const qp = a.q + sl * a.in_ss;
  const double* const dqp = a.dq + sl * a.in_ss;
  const double* const tp = a.tau + sl * a.in_ss;
  bool ok = a.status[sl] > 0;
#pragma unroll 4
  for (int i = 0; i < n; ++i)
  {
    const double v = sp[i * a.seed_sj];
    ok = ok && vjp_finite(v) && vjp_finite(qp[i * a.in_sj]) && vjp_finite(dqp[i * a.in_sj]) && vjp_finite(tp[i * a.in_sj]);
    x[i * 64] = v;
  }
  a.status[sl] = ok ? 1 : -1;
  if (a.status_out) a.status_out[sl] = ok ? 1 : -1;
  const double qnan = __builtin_nan("");
  if (a.ddq && !ok)
  {
#pragma unroll 4
    for (int i = 0; i < n; ++i) a.ddq[sl * a.in_ss + i * a.in_sj] = qnan;
  }
#pragma unroll 1
  for (int kind = 0; kind < 3; ++kind)
  {
    const double* const X = kind == 0 ? a.dddq_dq : (kind == 1 ? a.dddq_dv : a.minv);
    double* const out = kind == 0 ? a.q_bar : (kind == 1 ? a.dq_bar : a.tau_bar);
    if (!out) continue;
    const double* const xp = X + sl;
    double* const op = out + sl * a.in_ss;
#pragma unroll 1
    for (int k = 0; k < n; ++k)
    {
      double r = 0.0;
#pragma unroll 4
      for (int i = 0; i < n; ++i) r = fma(xp[(int64_t)(i + n * k) * ld], x[i * 64], r);
      op[k * a.in_sj] = ok ? r : qnan;
    }
  }
}

__global__ __launch_bounds__(256) void k_vjp_seed_copy(const double* src, double* dst, int n, int64_t n_samples, int64_t ld, int64_t in_ss, int64_t in_sj)
{
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * n_samples) return;
  const int64_t i = e / n_samples, s = e - i * n_samples;
  dst[i * ld + s] = src[s * in_ss + i * in_sj];
}

template <int NJ>
hipError_t launch_vjp_nj(const RdynFwdDynVjpArgs& a, hipStream_t st)
{
  const size_t lds = a.staged ? (size_t)64 * (size_t)(a.staged | 1) * 8 : 0;
  hipLaunchKernelGGL((k_fwd_dyn_vjp<NJ>), dim3((unsigned)((a.n_samples + 63) / 64)), dim3(64), lds, st, a);
  return hipGetLastError();
}
}  // namespace

hipError_t rdyn_launch_forward_dynamics_vjp(int n_joints, const RdynFwdDynVjpArgs& a, hipStream_t st)
{
  if (a.n_samples <= 0) return hipSuccess;
  if (a.t.n_comps < 0 || a.t.n_comps > RDYN_MAX_COMPONENTS || (!a.q_bar && !a.dq_bar && !a.tau_bar)) return hipErrorInvalidValue;
#define CALL(N) launch_vjp_nj<N>(a, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}

hipError_t rdyn_launch_vjp_products(const RdynVjpProductArgs& a, hipStream_t st)
{
  if (a.n_samples <= 0) return hipSuccess;
  if (a.n < 1 || a.n > RDYN_MAX_JOINTS || a.ld < a.n_samples || !a.status || !a.q || !a.dq || !a.tau || !a.ddq_bar || (a.q_bar && !a.dddq_dq) || (a.dq_bar && !a.dddq_dv) ||
      (a.tau_bar && !a.minv))
    return hipErrorInvalidValue;
  const size_t lds = (size_t)a.n * 64 * sizeof(double);  // <= 16 KB
  hipLaunchKernelGGL(k_vjp_products, dim3((unsigned)((a.n_samples + 63) / 64)), dim3(64), lds, st, a);
  return hipGetLastError();
}

hipError_t rdyn_launch_vjp_seed_copy(const double* src, double* dst, int n, int64_t n_samples, int64_t ld, int64_t in_ss, int64_t in_sj, hipStream_t st)
{
  if (n_samples <= 0 || n < 1) return hipSuccess;
  if (!src || !dst || ld < n_samples) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_vjp_seed_copy, dim3((unsigned)((n * n_samples + 255) / 256)), dim3(256), 0, st, src, dst, n, n_samples, ld, in_ss, in_sj);
  return hipGetLastError();
}
