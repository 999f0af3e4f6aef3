// rdyn_fwd_dyn_vjp_body.h -- one reverse-mode product of the forward dynamics ddq = FD_c(q, dq, tau) of a chain swept in registers, shared
// by k_fwd_dyn_vjp (rdyn_fwd_dyn_vjp.hip: one product per sample) and k_rollout_adjoint (rdyn_rollout_adjoint.hip: one per integrator
// stage of every backward step, the adjoint state staying in registers between them).  With the seed ab on ddq:
//     w = M^-1 ab,   tau_bar = w,   q_bar = -(dtau_dq + diag d tau_c / d q)' w,   dq_bar = -(dtau_dv + diag d tau_c / d dq)' w,
// dtau_dq, dtau_dv the matrices of rdyn_joint_torque_derivatives at that very ddq (rdyn_fwd_dyn_deriv.hip has the definitions).
//   1  the component torque leaves the torque, then rdyn_fwd_dyn_body.inc: ddq, the Cholesky factor L of M, the pivot test
//   2  L y = ab, L' w = y while L is still in registers; L is dead from here on (k_fwd_dyn_deriv parks it in LDS for 2 n solves: this
//      evaluation needs one)
//   3  the primal torque sweep at that ddq (rdyn_joint_step.h; sin q / 1 - cos q are the body's)
//   4  the tangent columns of rdyn_tangent_step.h, one input joint at a time and both kinds: the rows of column k appear one by one in the
//      backward accumulation and go straight into the dot product with w -- no column, let alone a matrix, is ever held
//   5  the component slope (rdyn_component_row.h's rule, the outer side at a kink) times w_k on top, the sign
// Live across step 4: the primal sweep state (21 doubles per joint), w and the two result vectors.
#ifndef RDYN_FWD_DYN_VJP_BODY_H
#define RDYN_FWD_DYN_VJP_BODY_H
#include <hip/hip_runtime.h>
#include <type_traits>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_fwd_dyn_body.h"
#include "rdyn_component_row.h"
#include "rdyn_joint_step.h"
#include "rdyn_tangent_step.h"

namespace
{
// one sample's finite test of an input (NaN and +-inf fail)
__device__ __forceinline__ bool vjp_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }

// In, by chain joint: rhs = tau, ab = the seed on ddq (both 0 where the joint is no input joint); q_of(f, idx), dq_of(f, idx) = q, dq of
// chain joint f with input index idx >= 0 -- an array in registers (k_rollout_adjoint: the stage state) or a load where the value is
// used (k_fwd_dyn_vjp: 2 NJ doubles fewer across the sweeps).  Out: rhs = ddq, ab = tau_bar = w, qb = q_bar (want_q), vb = dq_bar
// (want_v); the flags are wave-uniform and change no bit of what is computed.  early(ok, rhs) runs once ddq and the verdict are known,
// before the sweeps: a caller that stores ddq does it there and rhs is dead behind the primal sweep.  Returns ok: false when a pivot
// failed or an input of the sample was not finite -- no output is to be used then.
template <int NJ, class QF, class DQF, class EARLY>
__device__ __forceinline__ bool fwd_dyn_vjp_eval(ChainPtr c, const RdynComponentTable& tb, QF q_of, DQF dq_of, double (&rhs)[NJ],
                                                 double (&ab)[NJ], double (&qb)[NJ], double (&vb)[NJ], bool want_q, bool want_v, EARLY early)
{
  bool fin = true;
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    const int idx = c->j[f].in_idx;
    qb[f] = vb[f] = 0.0;
    if (idx < 0) continue;
    const double qv = q_of(f, idx), dqv = dq_of(f, idx);
    fin = fin && vjp_finite(qv) && vjp_finite(dqv) && vjp_finite(rhs[f]) && vjp_finite(ab[f]);
    rhs[f] -= joint_component_torque(tb, idx, qv, dqv);
  }

#define RDYN_FWD_Q(f, idx) q_of(f, idx)
#define RDYN_FWD_DQ(f, idx) dq_of(f, idx)
#include "rdyn_fwd_dyn_body.inc"
#undef RDYN_FWD_Q
#undef RDYN_FWD_DQ
  // (in scope from here on: sv0, sv1 = sin q / 1 - cos q by chain joint, M = the factor, rhs = ddq, ok)

  // ---- w = L^-T L^-1 ab (identity rows for locked joints: their entries stay 0)
#pragma unroll
  for (int i = 0; i < NJ; ++i)
  {
    double v = ab[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v = fma(-M[TRI(i, k)], ab[k], v);
    ab[i] = v * M[TRI(i, i)];
  }
#pragma unroll
  for (int i = NJ - 1; i >= 0; --i)
  {
    double v = ab[i];
#pragma unroll
    for (int k = i + 1; k < NJ; ++k) v = fma(-M[TRI(k, i)], ab[k], v);
    ab[i] = v * M[TRI(i, i)];
  }
  const bool good = ok && fin;
  early(good, rhs);
  if (!want_q && !want_v) return good;  // wave-uniform

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
      const double dqf = J.in_idx >= 0 ? dq_of(f, J.in_idx) : 0.0;
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

  // ---- one column per input joint, reduced against w row by row: KIND 0 d / d q_k, KIND 1 d / d Dq_k
  auto columns = [&](auto kind_tag, double (&out)[NJ]) {
    constexpr int KIND = decltype(kind_tag)::value;
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
      double r = 0.0;  // column k of dtau . w, the rows from the tip down
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
        if (J.in_idx >= 0)
        {
          if (type == RDYN_REVOLUTE) r = fma(dot(u, dN), ab[f], r);
          else if (type == RDYN_PRISMATIC) r = fma(dot(u, dF), ab[f], r);
        }
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
      out[k] = -fma(joint_component_slope(tb, col, KIND, q_of(k, col), dqs[k]), ab[k], r);
    }
  };
  if (want_q) columns(std::integral_constant<int, 0>(), qb);
  if (want_v) columns(std::integral_constant<int, 1>(), vb);
  return good;
}
}  // namespace
#endif
