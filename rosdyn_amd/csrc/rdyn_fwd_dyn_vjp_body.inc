// rdyn_fwd_dyn_vjp_body.inc -- the body of one reverse-mode product of the forward dynamics (rdyn_fwd_dyn_vjp_body.h has the scheme and the
// arguments), included as text by its two forms so that the plain one compiles to exactly what it compiled to before the other existed.
// RDYN_VJP_PARAMS 0: fwd_dyn_vjp_eval.  1: fwd_dyn_vjp_params_eval -- the primal sweep runs whatever want_q and want_v say, the LINEAR
// twist recursion with the joint rates w runs beside it ((ov, vv) = the angular and linear velocity of the link per unit of the seed, own
// frame, about its origin), and link(f, J, omega, v, alpha, acc, ov, vv) is called once per chain link, base to tip, with the link's
// primal state at ddq.
// RDYN_VJP_EXT 1: fwd_dyn_vjp_ext_eval (RDYN_VJP_PARAMS 0) -- external link wrenches x (rdyn_ext_wrench.h) enter the evaluation through the
// link-wrench hook and the primal sweep at ddq through the same ext_link_wrench, so the KIND 0 term of joint k's own transform sees them;
// the KIND 0 columns carry the tangent of pl, the link origin in link coordinates (the only part of [-(e.lin + e.ang x pl); -e.ang] that
// depends on q), beside tangent_step and add -e.ang x dpl to dFo[f].  With want_e (wave-uniform) the twist recursion of the parameter
// form runs too and ext_out(link, vv, ov + pl x vv) is called once per chain link 1 .. NJ: -(d tau_E / d ext)' w of that link's record.
// The sample is not finite when a wrench entry it reads is not.
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
#if RDYN_VJP_EXT
  {
    uint64_t p = (uint64_t)x.rec;  // laundered once per evaluation (fwd_dyn_eval_ext says why)
    asm volatile("" : "+v"(p));
    x.rec = (const double*)p;
  }
  V3 pl = mk(0, 0, 0);
#define RDYN_FWD_LINK_WRENCH(f, R, t, fo, no)  \
  ext_link_wrench(x, f + 1, R, t, pl, fo, no); \
  fin = fin && vjp_finite(fo.x) && vjp_finite(fo.y) && vjp_finite(fo.z) && vjp_finite(no.x) && vjp_finite(no.y) && vjp_finite(no.z);
#else
#define RDYN_FWD_LINK_WRENCH(f, R, t, fo, no)
#endif
#include "rdyn_fwd_dyn_body.inc"
#undef RDYN_FWD_LINK_WRENCH
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
#if RDYN_VJP_EXT
  if (!want_q && !want_v && !want_e) return good;  // wave-uniform
#elif !RDYN_VJP_PARAMS
  if (!want_q && !want_v) return good;  // wave-uniform
#endif

  // ---- primal forward sweep at ddq: the state of every link, its net wrench
  double dqs[NJ];
  V3 W[NJ], VL[NJ], AL[NJ], AC[NJ], Fc[NJ], Nc[NJ];
#if RDYN_VJP_EXT
  V3 PL[NJ];  // the origin of link f + 1 in its own coordinates
#endif
  {
    V3 w = mk(0, 0, 0), vl = mk(0, 0, 0), al = mk(0, 0, 0);
    V3 acc = mk(-c->g[0], -c->g[1], -c->g[2]);  // base "acceleration" -g
#if RDYN_VJP_PARAMS
    V3 ov = mk(0, 0, 0), vv = mk(0, 0, 0);  // the twist of the link under the joint rates w = ab
#endif
#if RDYN_VJP_EXT
    V3 ov = mk(0, 0, 0), vv = mk(0, 0, 0);  // the same twist, carried with want_e alone
    pl = mk(0, 0, 0);
#endif
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
#if RDYN_VJP_PARAMS
      {
        const V3 vn = rotT(R, vv + cross(ov, t));
        ov = rotT(R, ov);
        vv = vn;
        if (J.type == RDYN_REVOLUTE) ov = axpy(ov, ld3(J.u), ab[f]);
        else if (J.type == RDYN_PRISMATIC) vv = axpy(vv, ld3(J.u), ab[f]);
        link(f, J, w, vl, al, acc, ov, vv);
      }
#endif
#if RDYN_VJP_EXT
      ext_link_wrench(x, f + 1, R, t, pl, Fc[f], Nc[f]);
      PL[f] = pl;
      if (want_e)
      {
        const V3 vn = rotT(R, vv + cross(ov, t));
        ov = rotT(R, ov);
        vv = vn;
        if (J.type == RDYN_REVOLUTE) ov = axpy(ov, ld3(J.u), ab[f]);
        else if (J.type == RDYN_PRISMATIC) vv = axpy(vv, ld3(J.u), ab[f]);
        ext_out(f + 1, vv, ov + cross(pl, vv));
      }
#endif
    }
  }
#if RDYN_VJP_PARAMS || RDYN_VJP_EXT
  if (!want_q && !want_v) return good;  // wave-uniform
#endif
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
#if RDYN_VJP_EXT
        V3 dpl = mk(0, 0, 0);  // the tangent of pl: R' of joint k differentiated, or its translation
        if (KIND == 0)
        {
          if (Jk.type == RDYN_REVOLUTE) dpl = cross(PL[k], ld3(Jk.u));
          else if (Jk.type == RDYN_PRISMATIC) dpl = ld3(Jk.u);
          ext_tangent_wrench(x, k + 1, dpl, dFo[k]);
        }
#endif
#pragma unroll
        for (int f = k + 1; f < NJ; ++f)
        {
          JointRef J = c->j[f];
          double R[9];
          V3 t;
          joint_transform(J, sv0[f], sv1[f], R, t);
          tangent_step(J, R, t, dqs[f], d);
          tangent_wrench(J, W[f], VL[f], d, dFo[f], dNo[f]);
#if RDYN_VJP_EXT
          if (KIND == 0)
          {
            dpl = rotT(R, dpl);
            ext_tangent_wrench(x, f + 1, dpl, dFo[f]);
          }
#endif
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
