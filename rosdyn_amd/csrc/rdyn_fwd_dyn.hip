// rdyn_fwd_dyn.hip -- batched forward dynamics: ddq = M(q)^-1 (tau - h(q, dq)) (rdyn_forward_dynamics; no counterpart in the
// reference, defined by getJointInertia, primitives_impl.h:1357-1379, and getJointTorqueNonLinearPart, :1274-1293).
//
//   k_fwd_dyn<NJ>   chains the unrolled kernels sweep (1 .. RDYN_MAX_SWEPT_JOINTS joints): ONE launch, one lane per sample, nothing
//     but the inputs and the result touches memory.
//       forward   the local-frame sweep of rdyn_local_sweep_body.inc's torque mode with DDq = 0: w, vl, al, acc per link and the
//                 link's net wrench about its origin (getWrench, :1240-1250); sin q / 1 - cos q are kept per joint (2 NJ doubles),
//                 the wrenches wait for the backward pass (6 NJ doubles)
//       backward  composite rigid bodies: the spatial inertia of everything downstream of joint j is ten numbers in link j + 1's
//                 frame (m, h = m c, I about the link origin), carried to the parent by the rebuilt joint transform together with the
//                 bias wrench; h_j = S_j . (wrench), and column j of M is S_l . (Ic_j S_j) for the joints l <= j upstream: the six
//                 numbers Ic_j S_j of every column already started ride along into the parent frame (6 (NJ - j) doubles while the
//                 wrenches of the links passed are released).  The packed lower triangle of M is NJ (NJ + 1) / 2 <= 55 doubles.
//       solve     unrolled Cholesky M = L L' in place, two triangular solves.  A joint that is not an input joint is locked at 0: its
//                 row and column are replaced by the identity's and its right-hand side by 0, so the factorisation stays branch-free.
//     The O(n) articulated-body algorithm keeps a 6 x 6 articulated inertia (21 doubles) per link alive between its second and third
//     pass: 420 registers at 10 joints against 110 for the packed M, and at n <= 10 the factorisation is ~n^3 / 6 <= 170 fma.
//   k_fwd_solve     more than RDYN_MAX_SWEPT_JOINTS input joints: k_long_inertia (rdyn_long_local.hip) and the wrench recursion
//     (rdyn_long_kin.hip) write an element-major chunk image [M | h] (image[e][s]: every access of a wave is 512 contiguous bytes);
//     this kernel factorises it in place, one lane per sample, left-looking by columns: row j of L and the solution vector sit in
//     wave-private LDS ([k][lane]: a lane reads and writes its own column, no barrier), so the inner product of an entry costs one
//     global (L2 / Infinity Cache) and one LDS load per term.
// Status: 1 solved; -1 a Cholesky pivot (the squared diagonal entry of L, as in rdyn_ik.hip) at most 1e-10 trace(M) -- the sample's ddq
// is quiet NaN.
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_record_stage.h"

namespace
{
#define RDYN_FWD_PIVOT_FLOOR 1e-10  // rdyn_ik.hip's RDYN_IK_PIVOT_FLOOR
#define TRI(i, j) ((i) * ((i) + 1) / 2 + (j))  // lower triangle, i >= j

// parent -> child transform of a joint from its saved sin q / 1 - cos q (revolute) or q (prismatic)
__device__ __forceinline__ void joint_transform(JointRef J, double s0, double s1, double (&R)[9], V3& t)
{
  t = ld3(J.t);
  if (J.type == RDYN_REVOLUTE)
  {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = fma(s0, J.B[i], fma(s1, J.C[i], J.A[i]));
  }
  else
  {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = J.A[i];
    if (J.type == RDYN_PRISMATIC) t = axpy(t, ld3(J.up), s0);
  }
}

template <int NJ>
__global__ __launch_bounds__(64) void k_fwd_dyn(const RdynFwdDynArgs a)
{
  ChainPtr c = as_const(a.chain);
  const int lane = threadIdx.x;
  const int64_t s_wave = (int64_t)blockIdx.x * 64;
  const int64_t s = s_wave + lane;
  if (s >= a.n_samples) return;
  const bool stg = a.staged && a.n_samples - s_wave >= 64;  // wave-uniform: a full wave's records leave in whole lines
  const double* __restrict__ qp = a.q + s * a.in_ss;
  const double* __restrict__ dqp = a.dq + s * a.in_ss;
  const double* tp = a.tau + s * a.in_ss;  // (may alias ddq: every entry is read before the first store)

  double rhs[NJ];
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    const int idx = c->j[f].in_idx;
    rhs[f] = idx >= 0 ? tp[idx * a.in_sj] : 0.0;
  }

  // ---- forward: velocities, bias accelerations and the net wrench of every link in its own frame (DDq = 0)
  V3 w = mk(0, 0, 0), vl = mk(0, 0, 0), al = mk(0, 0, 0);
  V3 acc = mk(-c->g[0], -c->g[1], -c->g[2]);  // base "acceleration" -g
  double sv0[NJ], sv1[NJ];
  V3 Fo[NJ], No[NJ];
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    JointRef J = c->j[f];
    const int type = J.type;
    const int idx = J.in_idx;
    double qf = 0.0, dqf = 0.0;
    if (idx >= 0)
    {
      qf = qp[idx * a.in_sj];
      dqf = dqp[idx * a.in_sj];
    }
    if (type == RDYN_REVOLUTE)
    {
      double sn, cs;
      rdyn_sincos(qf, &sn, &cs);
      sv0[f] = sn;
      sv1[f] = 1.0 - cs;
    }
    else
    {
      sv0[f] = qf;
      sv1[f] = 0.0;
    }
    double R[9];
    V3 t;
    joint_transform(J, sv0[f], sv1[f], R, t);
    {
      const V3 wn = rotT(R, w);
      const V3 vn = rotT(R, vl + cross(w, t));
      const V3 aln = rotT(R, al);
      const V3 an = rotT(R, acc + cross(al, t));
      w = wn; vl = vn; al = aln; acc = an;
    }
    const V3 u = ld3(J.u);
    if (type == RDYN_REVOLUTE)
    {
      acc = axpy(acc, cross(vl, u), dqf);
      al = axpy(al, cross(w, u), dqf);
      w = axpy(w, u, dqf);
    }
    else if (type == RDYN_PRISMATIC)
    {
      acc = axpy(acc, cross(w, u), dqf);
      vl = axpy(vl, u, dqf);
    }
    const RDYN_CONST_AS double* pi = J.pi;
    const double m = pi[0];
    const V3 h = ld3(pi + 1);
    const V3 d = acc + cross(w, vl);
    Fo[f] = axpy(cross(al, h) + cross(w, cross(w, h)), d, m);
    No[f] = symv(pi + 4, al) + cross(w, symv(pi + 4, w)) + cross(h, d);
  }

  // ---- backward: composite bodies, bias torques, the columns of M
  double M[NJ * (NJ + 1) / 2];
  V3 cF[NJ], cN[NJ];  // column f: the momentum of composite body f under joint f's unit twist, in the current frame
  double cm = 0.0, cI[6] = {0, 0, 0, 0, 0, 0};
  V3 ch = mk(0, 0, 0), F = mk(0, 0, 0), N = mk(0, 0, 0);
  double trace = 0.0;
#pragma unroll
  for (int j = NJ - 1; j >= 0; --j)
  {
    JointRef J = c->j[j];
    const int type = J.type;
    const bool act = J.in_idx >= 0;
    const RDYN_CONST_AS double* pi = J.pi;
    cm += pi[0];
    ch = ch + ld3(pi + 1);
#pragma unroll
    for (int i = 0; i < 6; ++i) cI[i] += pi[4 + i];
    F = F + Fo[j];
    N = N + No[j];
    const V3 u = ld3(J.u);
    // momentum under the unit twist (lin, ang): F = m lin + ang x h, N = h x lin + I ang
    if (type == RDYN_REVOLUTE)
    {
      cF[j] = cross(u, ch);
      cN[j] = symv(cI, u);
    }
    else if (type == RDYN_PRISMATIC)
    {
      cF[j] = mk(cm * u.x, cm * u.y, cm * u.z);
      cN[j] = cross(ch, u);
    }
    else
    {
      cF[j] = mk(0, 0, 0);
      cN[j] = mk(0, 0, 0);
    }
    double hj = 0.0;
    if (type == RDYN_REVOLUTE) hj = dot(u, N);
    else if (type == RDYN_PRISMATIC) hj = dot(u, F);
    rhs[j] = act ? rhs[j] - hj : 0.0;
#pragma unroll
    for (int f = j; f < NJ; ++f)
    {
      double v = 0.0;
      if (type == RDYN_REVOLUTE) v = dot(u, cN[f]);
      else if (type == RDYN_PRISMATIC) v = dot(u, cF[f]);
      const bool both = act && c->j[f].in_idx >= 0;
      M[TRI(f, j)] = both ? v : (f == j ? 1.0 : 0.0);
    }
    if (act) trace += M[TRI(j, j)];
    if (j == 0) break;
    // into the parent's frame: x_parent = R x + t
    double R[9];
    V3 t;
    joint_transform(J, sv0[j], sv1[j], R, t);
    {
      const V3 Fp = rot(R, F);
      N = rot(R, N) + cross(t, Fp);
      F = Fp;
    }
#pragma unroll
    for (int f = j; f < NJ; ++f)
    {
      const V3 Fp = rot(R, cF[f]);
      cN[f] = rot(R, cN[f]) + cross(t, Fp);
      cF[f] = Fp;
    }
    {
      // m, h = m c, I about the origin: h' = R h + m t, I' = R I R' + (m |t|^2 + 2 t.hb) 1 - (m t t' + t hb' + hb t'), hb = R h
      const V3 hb = rot(R, ch);
      const V3 r0 = mk(R[0], R[1], R[2]), r1 = mk(R[3], R[4], R[5]), r2 = mk(R[6], R[7], R[8]);
      const V3 c0 = symv(cI, r0), c1 = symv(cI, r1), c2 = symv(cI, r2);
      const double tr = cm * dot(t, t) + 2.0 * dot(t, hb);
      cI[0] = dot(r0, c0) + tr - (cm * t.x * t.x + 2.0 * t.x * hb.x);
      cI[1] = dot(r0, c1) - (cm * t.x * t.y + t.x * hb.y + hb.x * t.y);
      cI[2] = dot(r0, c2) - (cm * t.x * t.z + t.x * hb.z + hb.x * t.z);
      cI[3] = dot(r1, c1) + tr - (cm * t.y * t.y + 2.0 * t.y * hb.y);
      cI[4] = dot(r1, c2) - (cm * t.y * t.z + t.y * hb.z + hb.y * t.z);
      cI[5] = dot(r2, c2) + tr - (cm * t.z * t.z + 2.0 * t.z * hb.z);
      ch = axpy(hb, t, cm);
    }
  }

  // ---- M = L L' in place (the diagonal holds 1 / L_jj), L y = rhs, L' x = y
  const double floor = RDYN_FWD_PIVOT_FLOOR * trace;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
  {
    double d = M[TRI(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) d = fma(-M[TRI(j, k)], M[TRI(j, k)], d);
    ok = ok && (c->j[j].in_idx < 0 || d > floor);
    const double inv = 1.0 / sqrt(d);
    M[TRI(j, j)] = inv;
#pragma unroll
    for (int i = j + 1; i < NJ; ++i)
    {
      double v = M[TRI(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) v = fma(-M[TRI(i, k)], M[TRI(j, k)], v);
      M[TRI(i, j)] = v * inv;
    }
  }
#pragma unroll
  for (int i = 0; i < NJ; ++i)
  {
    double v = rhs[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v = fma(-M[TRI(i, k)], rhs[k], v);
    rhs[i] = v * M[TRI(i, i)];
  }
#pragma unroll
  for (int i = NJ - 1; i >= 0; --i)
  {
    double v = rhs[i];
#pragma unroll
    for (int k = i + 1; k < NJ; ++k) v = fma(-M[TRI(k, i)], rhs[k], v);
    rhs[i] = v * M[TRI(i, i)];
  }

  if (a.status) a.status[s] = ok ? 1 : -1;
  const double qnan = __builtin_nan("");
  SmallRecords sm;
  if (stg)
  {
    extern __shared__ __attribute__((aligned(16))) char fwd_stage_lds[];
    sm.init(fwd_stage_lds, c->n_active, lane);
  }
  double* const op = a.ddq + s * a.in_ss;
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    const int idx = c->j[f].in_idx;
    if (idx < 0) continue;
    const double v = ok ? rhs[f] : qnan;
    if (stg) sm.put(idx, v);
    else op[idx * a.in_sj] = v;
  }
  if (stg) sm.copy_out(a.ddq + s_wave * a.in_ss, lane);
}

// element (i, j) of the lane's M at image[(i n + j) ld], h_i at image[(n n + i) ld]; both triangles of M are present, the lower one is used
__global__ __launch_bounds__(64) void k_fwd_solve(const RdynFwdSolveArgs a)
{
  extern __shared__ __attribute__((aligned(16))) double fwd_lds[];  // [2][n][64]: row j of L | the solution vector
  const int n = a.n;
  const int lane = threadIdx.x;
  const int64_t sl = (int64_t)blockIdx.x * 64 + lane;  // sample of the chunk
  if (sl >= a.n_samples) return;
  const int64_t ld = a.ld;
  double* const G = a.image + sl;
  double* const row = fwd_lds + lane;
  double* const y = fwd_lds + n * 64 + lane;
  const double* tp = a.tau + sl * a.in_ss;  // (may alias ddq: read whole before the first store)
  double* const op = a.ddq + sl * a.in_ss;

  double trace = 0.0;
#pragma unroll 4
  for (int i = 0; i < n; ++i)
  {
    trace += G[(int64_t)(i * n + i) * ld];
    y[i * 64] = tp[i * a.in_sj] - G[(int64_t)(n * n + i) * ld];
  }
  const double floor = RDYN_FWD_PIVOT_FLOOR * trace;
  bool ok = true;
#pragma unroll 1
  for (int j = 0; j < n; ++j)
  {
    double d = G[(int64_t)(j * n + j) * ld];
#pragma unroll 4
    for (int k = 0; k < j; ++k)
    {
      const double l = G[(int64_t)(j * n + k) * ld];
      row[k * 64] = l;
      d = fma(-l, l, d);
    }
    ok = ok && d > floor;
    const double inv = 1.0 / sqrt(d);
    G[(int64_t)(j * n + j) * ld] = inv;
#pragma unroll 1
    for (int i = j + 1; i < n; ++i)
    {
      double* const gi = G + (int64_t)(i * n) * ld;
      double v = gi[(int64_t)j * ld];
#pragma unroll 4
      for (int k = 0; k < j; ++k) v = fma(-gi[(int64_t)k * ld], row[k * 64], v);
      gi[(int64_t)j * ld] = v * inv;
    }
  }
#pragma unroll 1
  for (int i = 0; i < n; ++i)
  {
    const double* const gi = G + (int64_t)(i * n) * ld;
    double v = y[i * 64];
#pragma unroll 4
    for (int k = 0; k < i; ++k) v = fma(-gi[(int64_t)k * ld], y[k * 64], v);
    y[i * 64] = v * gi[(int64_t)i * ld];
  }
#pragma unroll 1
  for (int i = n - 1; i >= 0; --i)
  {
    double v = y[i * 64];
#pragma unroll 4
    for (int k = i + 1; k < n; ++k) v = fma(-G[(int64_t)(k * n + i) * ld], y[k * 64], v);
    y[i * 64] = v * G[(int64_t)(i * n + i) * ld];
  }
  if (a.status) a.status[sl] = ok ? 1 : -1;
  const double qnan = __builtin_nan("");
#pragma unroll 4
  for (int i = 0; i < n; ++i) op[i * a.in_sj] = ok ? y[i * 64] : qnan;
}

template <int NJ>
hipError_t launch_fwd_nj(const RdynFwdDynArgs& a, hipStream_t st)
{
  const size_t lds = a.staged ? (size_t)64 * (size_t)(a.staged | 1) * 8 : 0;
  hipLaunchKernelGGL((k_fwd_dyn<NJ>), dim3((unsigned)((a.n_samples + 63) / 64)), dim3(64), lds, st, a);
  return hipGetLastError();
}
}  // namespace

hipError_t rdyn_launch_forward_dynamics(int n_joints, const RdynFwdDynArgs& a, hipStream_t st)
{
  if (a.n_samples <= 0) return hipSuccess;
  switch (n_joints)
  {
  case 1: return launch_fwd_nj<1>(a, st);
  case 2: return launch_fwd_nj<2>(a, st);
  case 3: return launch_fwd_nj<3>(a, st);
  case 4: return launch_fwd_nj<4>(a, st);
  case 5: return launch_fwd_nj<5>(a, st);
  case 6: return launch_fwd_nj<6>(a, st);
  case 7: return launch_fwd_nj<7>(a, st);
  case 8: return launch_fwd_nj<8>(a, st);
  case 9: return launch_fwd_nj<9>(a, st);
  case 10: return launch_fwd_nj<10>(a, st);
  default: return hipErrorInvalidValue;
  }
}

hipError_t rdyn_launch_forward_solve(const RdynFwdSolveArgs& a, hipStream_t st)
{
  if (a.n_samples <= 0) return hipSuccess;
  if (a.n < 1 || a.n > RDYN_MAX_JOINTS || a.ld < a.n_samples) return hipErrorInvalidValue;
  const size_t lds = (size_t)2 * a.n * 64 * sizeof(double);  // <= 32 KB
  hipLaunchKernelGGL(k_fwd_solve, dim3((unsigned)((a.n_samples + 63) / 64)), dim3(64), lds, st, a);
  return hipGetLastError();
}
