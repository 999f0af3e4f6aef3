// rdyn_long_ik.hip -- batched local inverse kinematics of chains with more input joints than k_local_ik holds (11 .. RDYN_MAX_JOINTS
// chain joints, more than RDYN_MAX_SWEPT_JOINTS input joints: no reduced companion).
//
// Reference: Chain::computeLocalIk / computeWeigthedLocalIk, primitives_impl.h:1398-1468 (the loop of rdyn_ik.hip: frames -> e ->
// |w o e| < toll? -> tool Jacobian -> bound-constrained QP -> sol += dq).  k_local_ik keeps every per-joint quantity in registers
// with its joint loops unrolled; at 32 joints its packed H alone is 528 doubles.  Here, as in rdyn_long_kin.hip, the link loop is
// rolled (joint f's constants by scalar loads at a wave-uniform offset into RdynLongChainConst) and the per-variable state lives in
// wave-private LDS laid out [slot][variable][lane] (bank-conflict free): slots 0..5 the weighted Jacobian column a_k, slot 6 the
// step dq_k.  The iterate itself is kept in the caller's sol record.
//
// QP.  With A = diag(sqrt w) J (6 x n) and b = sqrt(w) o e the update minimises 1/2 |A dq - b|^2 + 1/2 lambda^2 |dq|^2 subject to
// q_min - sol <= dq <= q_max - sol, i.e. H = A'A + lambda^2 I = J'WJ + lambda^2 I and f = -J'We of the reference.  A primal active set
// over the bounds (two bit masks per lane), started at the feasible dq0 = clamp(0, q_min - sol, q_max - sol).  For a working set
// with free variables F and bound variables B the minimiser over F follows from the push-through identity
//     dq_F = (A_F'A_F + lambda^2 I)^-1 A_F' r = A_F' S_F^-1 r,   S_F = lambda^2 I + A_F A_F' (6 x 6),   r = b - A_B dq_B,
// so every solve is one 6 x 6 Cholesky in registers whatever n is (the Woodbury form H^-1 = (I - A'S^-1 A) / lambda^2 would cancel
// catastrophically for small lambda).  An infeasible step is cut at the first bound it meets (ratio test) and that variable joins
// B; a feasible one is taken whole and the multipliers of B are the gradient entries g_B = A_B'(A dq - b) + lambda^2 dq_B: the
// most violated one leaves B, none -> optimal.  H is positive definite, so the minimiser is unique and equals k_local_ik's
// (Goldfarb-Idnani) up to rounding.
//
// Statuses as in k_local_ik: 1 converged, 0 not within max_iter, -1 H not positive definite, -2 q_min > q_max, -3 QP guard.
// H = A'A + lambda^2 I has the eigenvalue lambda^2 as soon as n > 6, so k_local_ik's pivot rule (a Cholesky pivot of H at most
// 1e-10 trace(H)) becomes lambda^2 <= 1e-10 trace(H): in particular every undamped update is -1.  A negative weight makes A'A
// indefinite; this route reports it as -1 too (k_local_ik factorises J'WJ as it comes).  Fixed joints may be listed as inputs, so
// n (the moving ones) may be 6 or fewer here; the same floor then applies to S_F (a pivot at most 1e-10 trace(S_F) -> -1), which
// with lambda^2 below it is singular as soon as fewer than six variables are free.  k_local_ik solves such an undamped H_FF.
#include <hip/hip_runtime.h>
#include <cfloat>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_rotvec.h"
#include "rdyn_launch_util.h"
#include "rdyn_long_common.h"

namespace
{

#define RDYN_LONG_IK_PIVOT_FLOOR 1e-10  // k_local_ik's RDYN_IK_PIVOT_FLOOR
#define TRI6(i, j) ((i) * ((i) + 1) / 2 + (j))  // lower triangle of a 6 x 6, i >= j
constexpr int kLongIkSlots = 7;                 // LDS doubles per variable and lane

__device__ __forceinline__ double dot6(const double (&x)[6], const double (&y)[6])
{
  return fma(x[0], y[0], fma(x[1], y[1], fma(x[2], y[2], fma(x[3], y[3], fma(x[4], y[4], x[5] * y[5])))));
}

// One pose per lane, one wave per workgroup (poses need different numbers of updates).
__global__ __launch_bounds__(64) void k_long_ik(const RdynLongIkArgs a)
{
  extern __shared__ double ik_lds[];
  LongChainPtr c = as_const_long(a.chain_long);
  const int nj = c->n_joints, n = a.n_var;
  const int64_t s = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (s >= a.n_samples) return;
  const JointState js = {ik_lds + threadIdx.x, n, 64};  // slots 0..5: a variable's column, 6: its step
  auto ld_col = [&](int k, double (&ak)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) ak[i] = js.at(i, k);
  };

  // target frame, column-major 3x4 [R | p]
  double Ra[9];  // row-major
  const double* __restrict__ tp = a.T_target + s * a.tt_ss;
#pragma unroll
  for (int cc = 0; cc < 3; ++cc)
#pragma unroll
    for (int r = 0; r < 3; ++r) Ra[r * 3 + cc] = tp[(int64_t)(cc * 3 + r) * a.tt_se];
  const V3 pa = mk(tp[9 * a.tt_se], tp[10 * a.tt_se], tp[11 * a.tt_se]);

  // the iterate lives in the caller's record (sol may alias the seeds)
  const double* seed = a.seed + s * a.in_ss;
  double* sol = a.sol + s * a.in_ss;
#pragma unroll 1
  for (int i = 0; i < c->n_active; ++i) sol[i * a.in_sj] = seed[i * a.in_sj];  // :1403
  auto sol_of = [&](int k) -> double& { return sol[a.var_in[k] * a.in_sj]; };

  const double w0 = a.weight[0], w1 = a.weight[1], w2 = a.weight[2], w3 = a.weight[3], w4 = a.weight[4], w5 = a.weight[5];
  const bool neg_weight = w0 < 0.0 || w1 < 0.0 || w2 < 0.0 || w3 < 0.0 || w4 < 0.0 || w5 < 0.0;
  const double sw[6] = {sqrt(fmax(w0, 0.0)), sqrt(fmax(w1, 0.0)), sqrt(fmax(w2, 0.0)),
                        sqrt(fmax(w3, 0.0)), sqrt(fmax(w4, 0.0)), sqrt(fmax(w5, 0.0))};
  const double lam2 = a.damping * a.damping;

  int status = 0, it = 0;
  for (;; ++it)
  {
    // ---- frames at sol; z_k and p_k of every variable parked in its column slots
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    V3 p = mk(0, 0, 0);
    int k = 0;
#pragma unroll 1
    for (int f = 0; f < nj; ++f)
    {
      JointRef J = c->j[f];
      const int idx = J.in_idx;
      V3 z, d;
      frame_step(J, idx >= 0 ? sol[idx * a.in_sj] : 0.0, R, p, z, d);
      if (idx >= 0 && J.type != RDYN_FIXED)
      {
        js.put3(0, k, p);
        js.put3(3, k, z);
        ++k;
      }
    }
    // ---- getFrameDistance(T_target, T_tool) (frame_distance.h:44-49)
    double Rab[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) Rab[r * 3 + cc] = fma(Ra[0 + r], R[0 + cc], fma(Ra[3 + r], R[3 + cc], Ra[6 + r] * R[6 + cc]));
    const V3 el = pa - p;
    const V3 rv = rot(Ra, rotation_vector(Rab));
    const V3 ea = mk(-rv.x, -rv.y, -rv.z);
    const V3 wl = mk(w0 * el.x, w1 * el.y, w2 * el.z), wa = mk(w3 * ea.x, w4 * ea.y, w5 * ea.z);
    if (sqrt(dot(wl, wl) + dot(wa, wa)) < a.toll)  // :1409, :1446
    {
      status = 1;
      break;
    }
    if (it >= a.max_iter) break;
    if (neg_weight)
    {
      status = -1;
      break;
    }

    // ---- weighted Jacobian columns a_k = sqrt(w) o [z_k x (p_tool - p_k); z_k] (revolute), [z_k; 0] (prismatic)   (:944)
    double tr = 0.0, amax2 = 0.0;
    k = 0;
#pragma unroll 1
    for (int f = 0; f < nj; ++f)
    {
      JointRef J = c->j[f];
      if (J.in_idx < 0 || J.type == RDYN_FIXED) continue;
      const V3 po = js.get3(0, k), z = js.get3(3, k);
      V3 jl = z, ja = mk(0, 0, 0);
      if (J.type == RDYN_REVOLUTE)
      {
        jl = cross(z, p - po);
        ja = z;
      }
      const double ak[6] = {sw[0] * jl.x, sw[1] * jl.y, sw[2] * jl.z, sw[3] * ja.x, sw[4] * ja.y, sw[5] * ja.z};
#pragma unroll
      for (int i = 0; i < 6; ++i) js.at(i, k) = ak[i];
      const double a2 = dot6(ak, ak);
      tr += a2 + lam2;
      amax2 = fmax(amax2, a2);
      ++k;
    }
    if (n > 6 && lam2 <= RDYN_LONG_IK_PIVOT_FLOOR * tr)
    {
      status = -1;  // H = J'WJ + lambda^2 I numerically singular
      break;
    }
    const double b[6] = {sw[0] * el.x, sw[1] * el.y, sw[2] * el.z, sw[3] * ea.x, sw[4] * ea.y, sw[5] * ea.z};

    // ---- the feasible start dq0 = clamp(0, lo, hi); lo = q_min - sol, hi = q_max - sol  (ci0 of :1417-1418)
    unsigned actL = 0, actU = 0;
    bool crossed = false;
#pragma unroll 1
    for (k = 0; k < n; ++k)
    {
      const double q = sol_of(k), lo = a.q_min[k] - q, hi = a.q_max[k] - q;
      crossed = crossed || lo > hi;
      js.at(6, k) = fmin(fmax(0.0, lo), hi);
      if (lo > 0.0) actL |= 1u << k;
      else if (hi < 0.0) actU |= 1u << k;
    }
    if (crossed)
    {
      status = -2;
      break;
    }

    // ---- primal active set
    int qp = 0, released = -1;
    bool released_up = false;
    const int guard_max = 50 * (2 * n + 1);
#pragma unroll 1
    for (int guard = 0; n > 0; ++guard)
    {
      if (guard >= guard_max)
      {
        qp = -3;
        break;
      }
      const unsigned act = actL | actU;
      // S_F = lambda^2 I + A_F A_F',  r = b - A_B dq_B
      double S[21], r[6];
#pragma unroll
      for (int i = 0; i < 6; ++i)
      {
        r[i] = b[i];
#pragma unroll
        for (int j = 0; j <= i; ++j) S[TRI6(i, j)] = i == j ? lam2 : 0.0;
      }
#pragma unroll 1
      for (k = 0; k < n; ++k)
      {
        double ak[6];
        ld_col(k, ak);
        if ((act >> k) & 1u)
        {
          const double d = js.at(6, k);
#pragma unroll
          for (int i = 0; i < 6; ++i) r[i] = fma(-ak[i], d, r[i]);
        }
        else
        {
#pragma unroll
          for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) S[TRI6(i, j)] = fma(ak[i], ak[j], S[TRI6(i, j)]);
        }
      }
      // y = S_F^-1 r (Cholesky in registers); a pivot at most 1e-10 trace(S_F) counts as singular: with lambda^2 below that
      // floor S_F = A_F A_F' has rank |F| < 6 when fewer than six free variables are left (fixed joints among the inputs)
      double L[21], inv[6], y[6];
      const double floor_S = RDYN_LONG_IK_PIVOT_FLOOR * (S[TRI6(0, 0)] + S[TRI6(1, 1)] + S[TRI6(2, 2)] + S[TRI6(3, 3)] + S[TRI6(4, 4)] + S[TRI6(5, 5)]);
      bool ok = true;
#pragma unroll
      for (int j = 0; j < 6; ++j)
      {
        double d = S[TRI6(j, j)];
#pragma unroll
        for (int m = 0; m < j; ++m) d = fma(-L[TRI6(j, m)], L[TRI6(j, m)], d);
        ok = ok && d > floor_S;
        const double sd = sqrt(d);
        inv[j] = 1.0 / sd;
        L[TRI6(j, j)] = sd;
#pragma unroll
        for (int i = j + 1; i < 6; ++i)
        {
          double v = S[TRI6(i, j)];
#pragma unroll
          for (int m = 0; m < j; ++m) v = fma(-L[TRI6(i, m)], L[TRI6(j, m)], v);
          L[TRI6(i, j)] = v * inv[j];
        }
      }
      if (!ok)
      {
        qp = -1;
        break;
      }
#pragma unroll
      for (int i = 0; i < 6; ++i)
      {
        double v = r[i];
#pragma unroll
        for (int m = 0; m < i; ++m) v = fma(-L[TRI6(i, m)], y[m], v);
        y[i] = v * inv[i];
      }
#pragma unroll
      for (int i = 5; i >= 0; --i)
      {
        double v = y[i];
#pragma unroll
        for (int m = i + 1; m < 6; ++m) v = fma(-L[TRI6(m, i)], y[m], v);
        y[i] = v * inv[i];
      }
      // ratio test along dq_F -> A_F' y
      double alpha = 1.0;
      int blk = -1;
      bool blk_up = false;
#pragma unroll 1
      for (k = 0; k < n; ++k)
      {
        if ((act >> k) & 1u) continue;
        double ak[6];
        ld_col(k, ak);
        const double t = dot6(ak, y), d = js.at(6, k), q = sol_of(k);
        const double lo = a.q_min[k] - q, hi = a.q_max[k] - q;
        if (t < lo || t > hi)
        {
          const bool up = t > hi;
          const double al = fmax(0.0, ((up ? hi : lo) - d) / (t - d));
          if (al < alpha)
          {
            alpha = al;
            blk = k;
            blk_up = up;
          }
        }
      }
      if (blk >= 0)
      {
#pragma unroll 1
        for (k = 0; k < n; ++k)
        {
          if ((act >> k) & 1u) continue;
          double ak[6];
          ld_col(k, ak);
          const double d = js.at(6, k);
          js.at(6, k) = fma(alpha, dot6(ak, y) - d, d);
        }
        const double q = sol_of(blk);
        js.at(6, blk) = blk_up ? a.q_max[blk] - q : a.q_min[blk] - q;
        if (blk_up) actU |= 1u << blk;
        else actL |= 1u << blk;
        // the variable just released runs straight back into the bound it left (alpha = 0): its multiplier was rounding -- the
        // previous point is optimal.  Blocked at its OTHER bound it has moved (alpha > 0) and the iteration goes on.
        if (blk == released && blk_up == released_up) break;
        released = -1;
        continue;
      }
#pragma unroll 1
      for (k = 0; k < n; ++k)
      {
        if ((act >> k) & 1u) continue;
        double ak[6];
        ld_col(k, ak);
        js.at(6, k) = dot6(ak, y);
      }
      if (act == 0u) break;
      // multipliers of the bound variables: g_B = A_B'(A dq - b) + lambda^2 dq_B, >= 0 at a lower bound, <= 0 at an upper one
      double res[6] = {-b[0], -b[1], -b[2], -b[3], -b[4], -b[5]};
      double sum_ad = 0.0, dmax = 0.0;
#pragma unroll 1
      for (k = 0; k < n; ++k)
      {
        double ak[6];
        ld_col(k, ak);
        const double d = js.at(6, k);
#pragma unroll
        for (int i = 0; i < 6; ++i) res[i] = fma(ak[i], d, res[i]);
        sum_ad = fma(sqrt(dot6(ak, ak)), fabs(d), sum_ad);
        dmax = fmax(dmax, fabs(d));
      }
      const double thr = 16.0 * DBL_EPSILON * (sqrt(amax2) * (sum_ad + sqrt(dot6(b, b))) + lam2 * dmax);
      double worst = thr;
      int rel = -1;
#pragma unroll 1
      for (k = 0; k < n; ++k)
      {
        if (!((act >> k) & 1u)) continue;
        double ak[6];
        ld_col(k, ak);
        const double g = fma(lam2, js.at(6, k), dot6(ak, res));
        const double viol = ((actL >> k) & 1u) ? -g : g;
        if (viol > worst)
        {
          worst = viol;
          rel = k;
        }
      }
      if (rel < 0) break;
      released = rel;
      released_up = (actU >> rel) & 1u;
      actL &= ~(1u << rel);
      actU &= ~(1u << rel);
    }
    if (qp != 0)
    {
      status = qp;
      break;
    }
#pragma unroll 1
    for (k = 0; k < n; ++k) sol_of(k) += js.at(6, k);  // :1428
  }
  if (a.status) a.status[s] = status;
  if (a.iterations) a.iterations[s] = it;
}

}  // namespace

size_t rdyn_long_ik_lds_bytes(int n_var) { return (size_t)kLongIkSlots * n_var * 64 * sizeof(double); }

hipError_t rdyn_launch_long_ik(const RdynLongIkArgs& a, hipStream_t st)
{
  if (a.n_samples <= 0) return hipSuccess;
  if (a.n_var < 0 || a.n_var > RDYN_MAX_JOINTS) return hipErrorInvalidValue;
  const size_t lds = rdyn_long_ik_lds_bytes(a.n_var);
  if (lds > 64 * 1024)
  {
    hipError_t e = opt_in_lds_once<k_long_ik>();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_long_ik, dim3((unsigned)((a.n_samples + 63) / 64)), dim3(64), lds, st, a);
  return hipGetLastError();
}
