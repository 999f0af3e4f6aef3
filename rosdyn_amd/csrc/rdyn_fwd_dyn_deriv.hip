// rdyn_fwd_dyn_deriv.hip -- batched derivatives of the forward dynamics (rdyn_forward_dynamics_derivatives; no counterpart in the
// reference): with ddq = FD_c(q, dq, tau) = M^-1 (tau - tau_c(q, dq) - h(q, dq)) per sample
//     dddq_dq = -M^-1 (dtau_dq + diag d tau_c / d q),   dddq_dv = -M^-1 (dtau_dv + diag d tau_c / d dq),   minv = M^-1,
// dtau_dq, dtau_dv the matrices of rdyn_joint_torque_derivatives at that very ddq (the derivative of M ddq + h at fixed ddq: the chain
// rule's M^-1 (d M / d q) ddq term is inside dtau_dq).
//
//   k_fwd_dyn_deriv<NJ>   1 .. RDYN_MAX_SWEPT_JOINTS chain joints, one lane per sample, ONE launch, nothing but the inputs and the outputs
//     touches memory.
//       1  rdyn_fwd_dyn_body.inc (k_fwd_dyn's text, the component torque subtracted in front of it as in k_fwd_dyn_comp): ddq and the
//          Cholesky factor L of M by chain joint, identity rows for locked joints, 1 / L_jj on the diagonal.  ddq is stored, L moves to
//          wave-private LDS ([entry][lane]: a lane reads and writes its own column, 8 bytes per lane, conflict-free, no barrier) -- the
//          register file is about to fill with the primal state of the tangent sweep (21 doubles per joint).
//       2  the primal torque sweep at that ddq and the tangent columns, one input joint at a time: k_torque_deriv's text and helpers
//          (rdyn_tangent_step.h); sin q / 1 - cos q are the body's.
//       3  the moment a column is complete (NJ doubles in registers): the component slope on its diagonal entry, L y = c, L' x = y with L
//          from LDS (NJ^2 loads), -x stored or dropped into the wave's record tile.
//       4  minv from unit columns: column k starts at row k in the first solve and the second stops there -- the entries at and below the
//          diagonal, mirrored into the upper triangle: both triangles hold the same bits.
//     LDS per wave: NJ (NJ + 1) / 2 x 512 bytes of L (28 160 at 10 joints) and, for sample-major records of a full wave to line-aligned
//     outputs, the SmallRecords tile of k_torque_deriv (64 (n n | 1) doubles, 51 712 bytes at 10 input joints).
//   k_fwd_solve_columns   more input joints: after k_fwd_solve left L in the chunk image and k_long_torque_deriv wrote dtau_dq, dtau_dv
//     into the caller's matrices, this kernel solves them in place, k_fwd_solve's access pattern: one lane per sample, the column in
//     wave-private LDS, L from the element-major image (512 contiguous bytes per wave and access).
// A sample whose factorisation failed the pivot rule (status -1) gets quiet NaN in every entry.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_record_stage.h"
#include "rdyn_fwd_dyn_body.h"
#include "rdyn_component_row.h"
#include "rdyn_launch_util.h"
#include "rdyn_joint_step.h"
#include "rdyn_tangent_step.h"

namespace
{
// L y = x, L' x = y in place, L at Ll[TRI(i, k) * 64] with 1 / L_ii on the diagonal; x[i] = 0 for i < I0 on entry and only x[I0 ..] is
// valid on exit when I0 > 0 (a unit column of the inverse: the entries at and below its diagonal)
template <int NJ>
__device__ __forceinline__ void factor_solve(const double* Ll, double (&x)[NJ], int i0)
{
#pragma unroll
  for (int i = 0; i < NJ; ++i)
  {
    if (i < i0) continue;
    double v = x[i];
#pragma unroll
    for (int k = 0; k < i; ++k)
      if (k >= i0) v = fma(-Ll[TRI(i, k) * 64], x[k], v);
    x[i] = v * Ll[TRI(i, i) * 64];
  }
#pragma unroll
  for (int i = NJ - 1; i >= 0; --i)
  {
    if (i < i0) continue;
    double v = x[i];
#pragma unroll
    for (int k = i + 1; k < NJ; ++k) v = fma(-Ll[TRI(k, i) * 64], x[k], v);
    x[i] = v * Ll[TRI(i, i) * 64];
  }
}

template <int NJ>
__global__ __launch_bounds__(64) void k_fwd_dyn_deriv(const RdynFwdDynDerivArgs ad)
{
  const RdynFwdDynArgs& a = ad.f;
  ChainPtr c = as_const(a.chain);
  const int lane = threadIdx.x;
  const int64_t s_wave = (int64_t)blockIdx.x * 64;
  const int64_t s = s_wave + lane;
  if (s >= a.n_samples) return;
  const bool stg = ad.staged && a.n_samples - s_wave >= 64;  // wave-uniform: a full wave's records leave in whole lines
  const int n = c->n_active;
  const double* __restrict__ qp = a.q + s * a.in_ss;
  const double* __restrict__ dqp = a.dq + s * a.in_ss;
  const double* tp = a.tau + s * a.in_ss;  // (may alias ddq: every entry is read before the first store)
  extern __shared__ __attribute__((aligned(16))) char fdd_lds[];  // L: [NJ (NJ + 1) / 2][64] doubles | the record tile
  double* const Ll = (double*)fdd_lds + lane;
  SmallRecords sm;
  if (stg) sm.init(fdd_lds + NJ * (NJ + 1) / 2 * 64 * sizeof(double), n * n, lane);

  double rhs[NJ];
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    const int idx = c->j[f].in_idx;
    rhs[f] = idx >= 0 ? tp[idx * a.in_sj] : 0.0;
  }
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    const int idx = c->j[f].in_idx;
    if (idx >= 0) rhs[f] -= joint_component_torque(ad.t, idx, qp[idx * a.in_sj], dqp[idx * a.in_sj]);
  }

#define RDYN_FWD_Q(f, idx) qp[idx * a.in_sj]
#define RDYN_FWD_DQ(f, idx) dqp[idx * a.in_sj]
#define RDYN_FWD_LINK_WRENCH(f, R, t, fo, no)
#include "rdyn_fwd_dyn_body.inc"
#undef RDYN_FWD_LINK_WRENCH
#undef RDYN_FWD_Q
#undef RDYN_FWD_DQ
  // (in scope from here on: sv0, sv1 = sin q / 1 - cos q by chain joint, M = the factor, rhs = ddq, ok)

  if (a.status) a.status[s] = ok ? 1 : -1;
  const double qnan = __builtin_nan("");
  {
    double* const op = a.ddq + s * a.in_ss;
#pragma unroll
    for (int f = 0; f < NJ; ++f)
    {
      const int idx = c->j[f].in_idx;
      if (idx >= 0) op[idx * a.in_sj] = ok ? rhs[f] : qnan;
    }
  }
#pragma unroll
  for (int e = 0; e < NJ * (NJ + 1) / 2; ++e) Ll[e * 64] = M[e];

  if (ad.dddq_dq || ad.dddq_dv)  // wave-uniform
  {
    // ---- primal forward sweep at ddq: the state of every link, its net wrench
    double dqs[NJ];
    V3 W[NJ], VL[NJ], AL[NJ], AC[NJ], Fc[NJ], Nc[NJ];
    {
      V3 w = mk(0, 0, 0), vl = mk(0, 0, 0), al = mk(0, 0, 0);
      V3 acc = mk(-c->g[0], -c->g[1], -c->g[2]);  // base "acceleration" -g
#pragma unroll
      for (int f = 0; f < NJ; ++f)
      {
        JointRef J = c->j[f];
        const int idx = J.in_idx;
        const double dqf = idx >= 0 ? dqp[idx * a.in_sj] : 0.0;
        dqs[f] = dqf;
        double R[9];
        V3 t;
        joint_transform(J, sv0[f], sv1[f], R, t);
        primal_step(J, R, t, dqf, rhs[f], w, vl, al, acc);
        W[f] = w; VL[f] = vl; AL[f] = al; AC[f] = acc;
        link_wrench(J, w, vl, al, acc, Fc[f], Nc[f]);
      }
    }
    // ---- primal backward pass: Fc, Nc[f] = the wrench through joint f (everything downstream), about link f + 1's origin, own frame
#pragma unroll
    for (int f = NJ - 1; f >= 1; --f)
    {
      double R[9];
      V3 t;
      joint_transform(c->j[f], sv0[f], sv1[f], R, t);
      const V3 Fp = rot(R, Fc[f]);
      Nc[f - 1] = Nc[f - 1] + rot(R, Nc[f]) + cross(t, Fp);
      Fc[f - 1] = Fc[f - 1] + Fp;
    }

    // ---- one column per input joint: KIND 0 d / d q_k, KIND 1 d / d Dq_k
    auto columns = [&](auto kind_tag, double* out) {
      constexpr int KIND = decltype(kind_tag)::value;
      double* const op = out + s * ad.m_ss;
#pragma unroll
      for (int k = 0; k < NJ; ++k)
      {
        JointRef Jk = c->j[k];
        const int col = Jk.in_idx;
        if (col < 0) continue;
        V3 dFo[NJ], dNo[NJ];  // (entries k .. NJ - 1 are used)
        {
          Tangent d = tangent_seed(KIND, Jk.type, ld3(Jk.u), W[k], VL[k], AL[k], AC[k]);
          tangent_wrench(Jk, W[k], VL[k], d, dFo[k], dNo[k]);
#pragma unroll
          for (int f = k + 1; f < NJ; ++f)
          {
            JointRef J = c->j[f];
            double R[9];
            V3 t;
            joint_transform(J, sv0[f], sv1[f], R, t);
            tangent_step(J, R, t, dqs[f], d);
            tangent_wrench(J, W[f], VL[f], d, dFo[f], dNo[f]);
          }
        }
        double x[NJ];  // the column of dtau by chain joint (0 in the rows of locked joints)
        V3 dF = mk(0, 0, 0), dN = mk(0, 0, 0);
#pragma unroll
        for (int f = NJ - 1; f >= 0; --f)
        {
          JointRef J = c->j[f];
          const int type = J.type;
          const V3 u = ld3(J.u);
          if (f >= k)
          {
            dF = dF + dFo[f];
            dN = dN + dNo[f];
          }
          double v = 0.0;
          if (J.in_idx >= 0)
          {
            if (type == RDYN_REVOLUTE) v = dot(u, dN);
            else if (type == RDYN_PRISMATIC) v = dot(u, dF);
          }
          x[f] = v;
          if (f == 0) break;
          if (KIND == 0 && f == k)
          {
            // the derivative of joint k's own transform applied to the primal wrench it transmits
            if (type == RDYN_REVOLUTE)
            {
              dF = dF + cross(u, Fc[k]);
              dN = dN + cross(u, Nc[k]);
            }
            else if (type == RDYN_PRISMATIC)
              dN = dN + cross(u, Fc[k]);
          }
          double R[9];
          V3 t;
          joint_transform(J, sv0[f], sv1[f], R, t);
          const V3 Fp = rot(R, dF);
          dN = rot(R, dN) + cross(t, Fp);
          dF = Fp;
        }
        // ---- the column is complete: the component slope on its diagonal, both solves, negate, store
        x[k] += joint_component_slope(ad.t, col, KIND, qp[col * a.in_sj], dqp[col * a.in_sj]);
        factor_solve<NJ>(Ll, x, 0);
#pragma unroll
        for (int f = 0; f < NJ; ++f)
        {
          const int row = c->j[f].in_idx;
          if (row < 0) continue;
          const double v = ok ? -x[f] : qnan;
          const int e = row + n * col;
          if (stg) sm.put(e, v);
          else op[e * ad.m_se] = v;
        }
      }
      if (stg) sm.copy_out(out + s_wave * ad.m_ss, lane);
    };
    if (ad.dddq_dq) columns(std::integral_constant<int, 0>(), ad.dddq_dq);
    if (ad.dddq_dv) columns(std::integral_constant<int, 1>(), ad.dddq_dv);
  }

  if (!ad.minv) return;
  {
    double* const mp = ad.minv + s * ad.m_ss;
#pragma unroll
    for (int k = 0; k < NJ; ++k)
    {
      const int col = c->j[k].in_idx;
      if (col < 0) continue;
      double x[NJ];
#pragma unroll
      for (int f = 0; f < NJ; ++f) x[f] = f == k ? 1.0 : 0.0;
      factor_solve<NJ>(Ll, x, k);
#pragma unroll
      for (int f = k; f < NJ; ++f)
      {
        const int row = c->j[f].in_idx;
        if (row < 0) continue;
        const double v = ok ? x[f] : qnan;
        if (stg)
        {
          sm.put(row + n * col, v);
          sm.put(col + n * row, v);
        }
        else
        {
          mp[(row + n * col) * ad.m_se] = v;
          mp[(col + n * row) * ad.m_se] = v;
        }
      }
    }
    if (stg) sm.copy_out(ad.minv + s_wave * ad.m_ss, lane);
  }
}

// ---- more input joints than the unrolled kernel sweeps: the columns of the caller's matrices solved in place ------------------------------
// element (i, j), i >= j, of the lane's L at image[(i n + j) ld], 1 / L_ii on the diagonal (k_fwd_solve, rdyn_fwd_dyn.hip)
__global__ __launch_bounds__(64) void k_fwd_solve_columns(const RdynFwdSolveColumnsArgs a)
{
  extern __shared__ __attribute__((aligned(16))) double fsc_lds[];  // [n][64]: the column
  const int n = a.n;
  const int lane = threadIdx.x;
  const int64_t sl = (int64_t)blockIdx.x * 64 + lane;  // sample of the chunk
  if (sl >= a.n_samples) return;
  const int64_t ld = a.ld;
  const double* const G = a.image + sl;
  double* const x = fsc_lds + lane;
  const bool ok = a.status[sl] > 0;
  const double qnan = __builtin_nan("");
  const double* const qp = a.q + sl * a.in_ss;
  const double* const dqp = a.dq + sl * a.in_ss;
#pragma unroll 1
  for (int kind = 0; kind < 3; ++kind)
  {
    double* const X = kind == 0 ? a.dddq_dq : (kind == 1 ? a.dddq_dv : a.minv);
    if (!X) continue;
    double* const xp = X + sl * a.m_ss;
#pragma unroll 1
    for (int k = 0; k < n; ++k)
    {
      const int i0 = kind == 2 ? k : 0;  // a unit column: the entries at and below the diagonal, mirrored into the upper triangle
      if (kind == 2)
      {
#pragma unroll 4
        for (int i = k; i < n; ++i) x[i * 64] = i == k ? 1.0 : 0.0;
      }
      else
      {
#pragma unroll 4
        for (int i = 0; i < n; ++i) x[i * 64] = xp[(int64_t)(i + n * k) * a.m_se];
        x[k * 64] += joint_component_slope(a.t, k, kind, qp[k * a.in_sj], dqp[k * a.in_sj]);
      }
#pragma unroll 1
      for (int i = i0; i < n; ++i)
      {
        const double* const gi = G + (int64_t)(i * n) * ld;
        double v = x[i * 64];
#pragma unroll 4
        for (int j = i0; j < i; ++j) v = fma(-gi[(int64_t)j * ld], x[j * 64], v);
        x[i * 64] = v * gi[(int64_t)i * ld];
      }
#pragma unroll 1
      for (int i = n - 1; i >= i0; --i)
      {
        double v = x[i * 64];
#pragma unroll 4
        for (int j = i + 1; j < n; ++j) v = fma(-G[(int64_t)(j * n + i) * ld], x[j * 64], v);
        x[i * 64] = v * G[(int64_t)(i * n + i) * ld];
      }
      if (kind == 2)
      {
#pragma unroll 4
        for (int i = k; i < n; ++i)
        {
          const double v = ok ? x[i * 64] : qnan;
          xp[(int64_t)(i + n * k) * a.m_se] = v;
          xp[(int64_t)(k + n * i) * a.m_se] = v;
        }
      }
      else
      {
#pragma unroll 4
        for (int i = 0; i < n; ++i) xp[(int64_t)(i + n * k) * a.m_se] = ok ? -x[i * 64] : qnan;
      }
    }
  }
}

template <int NJ>
hipError_t launch_fdd_nj(const RdynFwdDynDerivArgs& a, hipStream_t st)
{
  // the factor, and the record tile behind it: 28 160 + 51 712 bytes at 10 input joints
  const size_t lds = (size_t)NJ * (NJ + 1) / 2 * 64 * sizeof(double) + (a.staged ? (size_t)64 * (size_t)(a.staged | 1) * 8 : 0);
  if (lds > 64 * 1024)
  {
    hipError_t e = opt_in_lds_once<k_fwd_dyn_deriv<NJ>>();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((k_fwd_dyn_deriv<NJ>), dim3((unsigned)((a.f.n_samples + 63) / 64)), dim3(64), lds, st, a);
  return hipGetLastError();
}
}  // namespace

hipError_t rdyn_launch_forward_dynamics_derivatives(int n_joints, const RdynFwdDynDerivArgs& a, hipStream_t st)
{
  if (a.f.n_samples <= 0) return hipSuccess;
  if (a.t.n_comps < 0 || a.t.n_comps > RDYN_MAX_COMPONENTS || (!a.dddq_dq && !a.dddq_dv && !a.minv)) return hipErrorInvalidValue;
#define CALL(N) launch_fdd_nj<N>(a, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}

hipError_t rdyn_launch_forward_solve_columns(const RdynFwdSolveColumnsArgs& a, hipStream_t st)
{
  if (a.n_samples <= 0 || (!a.dddq_dq && !a.dddq_dv && !a.minv)) return hipSuccess;
  if (a.n < 1 || a.n > RDYN_MAX_JOINTS || a.ld < a.n_samples || !a.status || a.t.n_comps < 0 || a.t.n_comps > RDYN_MAX_COMPONENTS)
    return hipErrorInvalidValue;
  const size_t lds = (size_t)a.n * 64 * sizeof(double);  // <= 16 KB
  hipLaunchKernelGGL(k_fwd_solve_columns, dim3((unsigned)((a.n_samples + 63) / 64)), dim3(64), lds, st, a);
  return hipGetLastError();
}
