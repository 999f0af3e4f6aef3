// rdyn_fwd_dyn_param_vjp.hip -- the reverse-mode product of the forward dynamics with respect to the PARAMETERS of the model
// (rdyn_forward_dynamics_parameter_vjp; no counterpart in the reference): with ddq = FD_c(q, dq, tau), a seed ddq_bar per sample and
// w = M^-1 ddq_bar
//     pi_bar   = -Y(q, dq, ddq)' w     the inertial parameters, the columns of rdyn_regressor
//     comp_bar = -C(q, dq)' w          the component parameters, the columns of rdyn_components_regressor
// since tau = Y pi + C p at that ddq and M ddq_bar-wards is linear.  Neither Y nor C is formed.
//
//   k_fwd_dyn_param_vjp<NJ>   1 .. RDYN_MAX_SWEPT_JOINTS chain joints, one lane per sample, ONE launch.  The evaluation is
//     rdyn_fwd_dyn_vjp_body.h's with its link hook: the primal sweep at ddq hands over the state (omega, v, alpha, acc) of every link, and
//     beside it runs the LINEAR twist recursion with the joint rates w -- (ov, vv), the motion of the link per unit of the seed.  w' tau is
//     the power of the link wrenches on those twists; link_parameter_row (rdyn_fwd_dyn_vjp_body.h) differentiates it by the link's ten
//     parameters: the ten entries of Y' w of that link, about 60 flops, nothing kept.  A chain served through its reduced companion gets the
//     rows of its own links as X_f' g(body of f) (rdyn_chain.hpp), links upstream of the first input joint 0.
//     The sums over the samples: every wave reduces each column across its lanes by a fixed butterfly (a failed or absent sample adds
//     0) and lane 0 stores the wave's partial; k_param_sum_reduce adds the partials of a column in a fixed order (thread t takes the
//     waves t, t + 256, ...; then a tree) and k_param_sum_finish expands / copies / accumulates into the caller's vectors.  No
//     floating-point atomics: the same N, layout and device give the same bits.
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
// the sum over the wave's 64 lanes, the same bits in every lane: a butterfly, so the order of the additions is fixed
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

template <int NJ>
__global__ __launch_bounds__(64) void k_fwd_dyn_param_vjp(const RdynFwdDynParamVjpArgs a)
{
  ChainPtr c = as_const(a.v.chain);
  const int lane = threadIdx.x;
  const int64_t s_wave = (int64_t)blockIdx.x * 64;
  const bool live = s_wave + lane < a.v.n_samples;
  // (every lane runs to the end: the wave sums need all 64.  A lane past the batch evaluates the last sample and stores nothing.)
  const int64_t s = live ? s_wave + lane : a.v.n_samples - 1;
  const bool stg = a.v.staged && a.v.n_samples - s_wave >= 64;  // wave-uniform; a full wave

  const double* __restrict__ qp = a.v.q + s * a.v.in_ss;
  const double* __restrict__ dqp = a.v.dq + s * a.v.in_ss;
  double rhs[NJ], ab[NJ], qb[NJ], vb[NJ];
  {
    const double* __restrict__ tp = a.v.tau + s * a.v.in_ss;
    const double* sp = a.v.ddq_bar + s * a.v.in_ss;  // (may alias tau_bar: every entry is read before the first store)
#pragma unroll
    for (int f = 0; f < NJ; ++f)
    {
      const int idx = c->j[f].in_idx;
      rhs[f] = idx >= 0 ? tp[idx * a.v.in_sj] : 0.0;
      ab[f] = idx >= 0 ? sp[idx * a.v.in_sj] : 0.0;
    }
  }
  SmallRecords sm;
  if (stg)
  {
    extern __shared__ __attribute__((aligned(16))) char pvjp_stage_lds[];
    sm.init(pvjp_stage_lds, c->n_active, lane);
  }
  const double qnan = __builtin_nan("");
  const int64_t ow = s_wave * a.v.in_ss, oo = s * a.v.in_ss;
  const int cols_sw = 10 * NJ + a.n_comp_cols;
  double* const part = a.partials ? a.partials + (int64_t)blockIdx.x * cols_sw : nullptr;
  double* const prow = a.pi_bar ? a.pi_bar + s * a.pi_ss : nullptr;

  bool use = false;  // the sample counts: in range and evaluated
  const bool ok = fwd_dyn_vjp_params_eval<NJ>(
      c, a.v.t, [&](int, int idx) { return qp[idx * a.v.in_sj]; }, [&](int, int idx) { return dqp[idx * a.v.in_sj]; }, rhs, ab, qb, vb, false,
      false,
      [&](bool good, double (&ddq)[NJ]) {
        use = good && live;
        if (a.v.status && live) a.v.status[s] = good ? 1 : -1;
        // rows of the links that ride on the base (upstream of the first input joint of a chain served through its companion)
        if (a.expand && prow && live)
        {
#pragma unroll 1
          for (int ff = 0; ff < a.n_full; ++ff)
            if (a.red_of[ff] < 0)
              for (int p = 0; p < 10; ++p) prow[(10 * ff + p) * a.pi_sc] = good ? 0.0 : qnan;
        }
        if (!a.v.ddq) return;  // wave-uniform
        double v[NJ];
#pragma unroll
        for (int f = 0; f < NJ; ++f) v[f] = good ? ddq[f] : qnan;
        if (stg || live) put_record<NJ>(c, sm, stg, v, a.v.ddq + ow, a.v.ddq + oo, a.v.in_sj, lane);
      },
      [&](int f, JointRef J, V3 om, V3 vl, V3 al, V3 acc, V3 ov, V3 vv) {
        double g[10];
        link_parameter_row(om, vl, al, acc, ov, vv, g);
        if (part)
        {
#pragma unroll
          for (int p = 0; p < 10; ++p)
          {
            const double t = wave_sum(use ? g[p] : 0.0);
            if (lane == 0) part[10 * f + p] = t;
          }
        }
        if (!prow) return;  // wave-uniform
#pragma unroll
        for (int p = 0; p < 10; ++p) g[p] = use ? g[p] : qnan;
        if (!a.expand)
        {
          if (live)
          {
#pragma unroll
            for (int p = 0; p < 10; ++p) prow[(10 * f + p) * a.pi_sc] = g[p];
          }
          return;
        }
#pragma unroll 1
        for (int ff = 0; ff < a.n_full; ++ff)
        {
          if (a.red_of[ff] != f) continue;  // wave-uniform
          const double* const X = a.expand + ff * 100;
#pragma unroll 1
          for (int p = 0; p < 10; ++p)
          {
            double r = 0.0;
#pragma unroll
            for (int k = 0; k < 10; ++k) r = fma(X[k * 10 + p], g[k], r);
            if (live) prow[(10 * ff + p) * a.pi_sc] = r;
          }
        }
      });
#pragma unroll
  for (int f = 0; f < NJ; ++f) ab[f] = ok ? ab[f] : qnan;
  if (a.v.tau_bar && (stg || live)) put_record<NJ>(c, sm, stg, ab, a.v.tau_bar + ow, a.v.tau_bar + oo, a.v.in_sj, lane);

  // ---- the component columns: -row . w of the component's joint, the rows of rdyn_component_row.h at the sample's own state
  if (a.v.t.n_comps == 0 || (!a.comp_bar && !part)) return;  // wave-uniform
  double* const crow = a.comp_bar ? a.comp_bar + s * a.comp_ss : nullptr;
  int col = 0;
#pragma unroll 1
  for (int i = 0; i < a.v.t.n_comps; ++i)
  {
    const RdynComponent& cp = a.v.t.comps[i];
    double wj = 0.0;
#pragma unroll
    for (int f = 0; f < NJ; ++f)
      if (c->j[f].in_idx == cp.joint) wj = ab[f];
    double row[3];
    const int nc = component_row(cp, cp.type == RDYN_COMP_SPRING ? qp[cp.joint * a.v.in_sj] : dqp[cp.joint * a.v.in_sj], row);
    for (int k = 0; k < nc; ++k, ++col)
    {
      const double v = -(row[k] * wj);
      if (part)
      {
        const double t = wave_sum(use ? v : 0.0);
        if (lane == 0) part[10 * NJ + col] = t;
      }
      if (crow && live) crow[col * a.comp_sc] = use ? v : qnan;
    }
  }
}

// S[col] = the sum over the rows r < n_rows of x[r * row_stride + col * col_stride], rows whose status word is not 1 left out (status null:
// none is): thread t adds the rows t, t + 256, ... in that order, then a tree over the threads -- the same bits every time
__global__ __launch_bounds__(256) void k_param_sum_reduce(const double* x, int64_t n_rows, int64_t row_stride, int64_t col_stride,
                                                          const int32_t* status, double* S)
{
  __shared__ double red[256];
  const int col = blockIdx.x, t = threadIdx.x;
  const double* const xc = x + col * col_stride;
  double acc = 0.0;
  for (int64_t r = t; r < n_rows; r += 256)
    if (!status || status[r] == 1) acc += xc[r * row_stride];
  red[t] = acc;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1)
  {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  if (t == 0) S[col] = red[0];
}

// the caller's vectors from the sums of the swept chain: pi_sum[10 f + p] = sum_a X_f(a, p) S[10 r(f) + a] through a companion (0 for a
// link that rides on the base), S itself otherwise; comp_sum = the columns behind; accumulate: += instead of =
__global__ __launch_bounds__(256) void k_param_sum_finish(const RdynParamSumArgs a)
{
  const int o = blockIdx.x * 256 + threadIdx.x;
  const int P = 10 * a.n_full;
  if (o >= P + a.n_comp_cols) return;
  double v;
  double* dst;
  if (o < P)
  {
    dst = a.pi_sum ? a.pi_sum + o : nullptr;
    if (!a.expand) v = a.S[o];
    else
    {
      const int ff = o / 10, p = o - 10 * ff, r = a.red_of[ff];
      v = 0.0;
      if (r >= 0)
        for (int k = 0; k < 10; ++k) v = fma(a.expand[ff * 100 + k * 10 + p], a.S[10 * r + k], v);
    }
  }
  else
  {
    dst = a.comp_sum ? a.comp_sum + (o - P) : nullptr;
    v = a.S[10 * a.n_swept + (o - P)];
  }
  if (dst) *dst = a.accumulate ? *dst + v : v;
}

// ---- more input joints than the unrolled kernel sweeps: CORRECT BUT NOT FAST.  The host has tau_bar = w, ddq and the status of the whole
// batch from the chunked product (rdyn_api_dynamics.cpp) and, per chunk, the element-major image [Y | C] at that ddq (the writer of the
// wide normal equations); this kernel forms row[col] = -sum_j image[j * cnt + s][col] w_j, one lane per sample, 512 contiguous bytes per
// wave and access, j ascending whatever the chunk: the rows do not depend on the chunk size.
__global__ __launch_bounds__(64) void k_param_rows_from_image(const RdynParamProductArgs a)
{
  extern __shared__ __attribute__((aligned(16))) double ppr_lds[];  // [n][64]: w
  const int lane = threadIdx.x;
  const int64_t sl = (int64_t)blockIdx.x * 64 + lane;  // sample of the chunk
  if (sl >= a.cnt) return;
  double* const x = ppr_lds + lane;
  const double* const wp = a.tau_bar + sl * a.in_ss;
#pragma unroll 4
  for (int j = 0; j < a.n; ++j) x[j * 64] = wp[j * a.in_sj];
  const bool ok = a.status[sl] == 1;
  const double qnan = __builtin_nan("");
  const double* const ip = a.image + sl;
#pragma unroll 1
  for (int col = 0; col < a.P + a.K; ++col)
  {
    const bool comp = col >= a.P;
    double* const out = comp ? a.comp_rows : a.pi_rows;
    if (!out) continue;  // wave-uniform
    const double* const cp = ip + (int64_t)col * a.lda;
    double r = 0.0;
#pragma unroll 4
    for (int j = 0; j < a.n; ++j) r = fma(cp[(int64_t)j * a.cnt], x[j * 64], r);
    if (comp) out[sl * a.comp_ss + (col - a.P) * a.comp_sc] = ok ? -r : qnan;
    else out[sl * a.pi_ss + col * a.pi_sc] = ok ? -r : qnan;
  }
}

template <int NJ>
hipError_t launch_param_vjp_nj(const RdynFwdDynParamVjpArgs& a, hipStream_t st)
{
  const size_t lds = a.v.staged ? (size_t)64 * (size_t)(a.v.staged | 1) * 8 : 0;
  hipLaunchKernelGGL((k_fwd_dyn_param_vjp<NJ>), dim3((unsigned)((a.v.n_samples + 63) / 64)), dim3(64), lds, st, a);
  return hipGetLastError();
}
}  // namespace

hipError_t rdyn_launch_forward_dynamics_parameter_vjp(int n_joints, const RdynFwdDynParamVjpArgs& a, hipStream_t st)
{
  if (a.v.n_samples <= 0) return hipSuccess;
  if (a.v.t.n_comps < 0 || a.v.t.n_comps > RDYN_MAX_COMPONENTS || a.n_comp_cols < 0 || a.n_comp_cols > 3 * RDYN_MAX_COMPONENTS ||
      (a.expand && (a.n_full < 1 || a.n_full > RDYN_MAX_JOINTS)))
    return hipErrorInvalidValue;
#define CALL(N) launch_param_vjp_nj<N>(a, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}

hipError_t rdyn_launch_parameter_column_sums(const double* x, int64_t n_rows, int64_t row_stride, int64_t col_stride, const int32_t* status,
                                             int cols, double* S, hipStream_t st)
{
  if (cols <= 0) return hipSuccess;
  if (!x || !S || n_rows < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_param_sum_reduce, dim3((unsigned)cols), dim3(256), 0, st, x, n_rows, row_stride, col_stride, status, S);
  return hipGetLastError();
}

hipError_t rdyn_launch_parameter_sums_finish(const RdynParamSumArgs& a, hipStream_t st)
{
  if (!a.S || a.n_swept < 1 || a.n_full < 1 || a.n_full > RDYN_MAX_JOINTS || (!a.expand && a.n_full != a.n_swept)) return hipErrorInvalidValue;
  const int outs = 10 * a.n_full + a.n_comp_cols;
  hipLaunchKernelGGL(k_param_sum_finish, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t rdyn_launch_parameter_sums(const double* x, int64_t n_rows, int64_t row_stride, int64_t col_stride, const int32_t* status,
                                      const RdynParamSumArgs& a, hipStream_t st)
{
  if (a.n_swept < 1 || a.n_comp_cols < 0) return hipErrorInvalidValue;
  hipError_t e = rdyn_launch_parameter_column_sums(x, n_rows, row_stride, col_stride, status, 10 * a.n_swept + a.n_comp_cols, (double*)a.S, st);
  return e != hipSuccess ? e : rdyn_launch_parameter_sums_finish(a, st);
}

hipError_t rdyn_launch_parameter_rows_from_image(const RdynParamProductArgs& a, hipStream_t st)
{
  if (a.cnt <= 0) return hipSuccess;
  if (a.n < 1 || a.n > RDYN_MAX_JOINTS || a.lda < (int64_t)a.n * a.cnt || !a.image || !a.tau_bar || !a.status || a.P < 0 || a.K < 0) return hipErrorInvalidValue;
  const size_t lds = (size_t)a.n * 64 * sizeof(double);  // <= 16 KB
  hipLaunchKernelGGL(k_param_rows_from_image, dim3((unsigned)((a.cnt + 63) / 64)), dim3(64), lds, st, a);
  return hipGetLastError();
}
