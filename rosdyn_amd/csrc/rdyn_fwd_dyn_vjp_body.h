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
#include "rdyn_ext_wrench.h"

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
#define RDYN_VJP_PARAMS 0
#define RDYN_VJP_EXT 0
#include "rdyn_fwd_dyn_vjp_body.inc"
#undef RDYN_VJP_EXT
#undef RDYN_VJP_PARAMS
}

// The same product with a hook on every link of the primal sweep: what the gradients with respect to the model's parameters are made of
// (rdyn_fwd_dyn_param_vjp.hip, rdyn_rollout_adjoint_params.hip; rdyn_fwd_dyn_vjp_body.inc says what the hook is given).
template <int NJ, class QF, class DQF, class EARLY, class LINK>
__device__ __forceinline__ bool fwd_dyn_vjp_params_eval(ChainPtr c, const RdynComponentTable& tb, QF q_of, DQF dq_of, double (&rhs)[NJ],
                                                        double (&ab)[NJ], double (&qb)[NJ], double (&vb)[NJ], bool want_q, bool want_v, EARLY early,
                                                        LINK link)
{
#define RDYN_VJP_PARAMS 1
#define RDYN_VJP_EXT 0
#include "rdyn_fwd_dyn_vjp_body.inc"
#undef RDYN_VJP_EXT
#undef RDYN_VJP_PARAMS
}

// ---- with external link wrenches (rdyn_ext_wrench.h)
// the tangent of a link's wrench contribution [-(e.lin + e.ang x pl); -e.ang] along dpl, the tangent of pl: the force part alone has one
__device__ __forceinline__ void ext_tangent_wrench(const ExtEval& x, int link, V3 dpl, V3& dfo)
{
  V3 ea;
  if (x.one == 0)
  {
    const double* const p = x.rec + (int64_t)(6 * link + 3) * x.se;
    ea = mk(p[0], p[x.se], p[2 * x.se]);
  }
  else if (x.one == link + 1)
    ea = x.a;
  else
    return;
  dfo = dfo - cross(ea, dpl);
}

// The product of ddq = FD_E(q, dq, tau, ext) = FD_c(q, dq, tau - tau_E(q, ext)), x the wrenches of the evaluation
// (rdyn_fwd_dyn_vjp_ext.hip, rdyn_rollout_adjoint_ext.hip; rdyn_fwd_dyn_vjp_body.inc says what changes): q_bar gains -(d tau_E / d q)' w,
// and with want_e (wave-uniform) ext_out(link, lin, ang) is handed -(d tau_E / d ext)' w of every chain link 1 .. NJ, base to tip, behind
// early(): [lin; ang] in the layout of the link's wrench record.  tau_E is linear in ext: the record does not depend on the wrenches.
template <int NJ, class QF, class DQF, class EARLY, class EXTOUT>
__device__ __forceinline__ bool fwd_dyn_vjp_ext_eval(ChainPtr c, const RdynComponentTable& tb, QF q_of, DQF dq_of, double (&rhs)[NJ],
                                                     double (&ab)[NJ], double (&qb)[NJ], double (&vb)[NJ], bool want_q, bool want_v, EARLY early,
                                                     ExtEval x, bool want_e, EXTOUT ext_out)
{
#define RDYN_VJP_PARAMS 0
#define RDYN_VJP_EXT 1
#include "rdyn_fwd_dyn_vjp_body.inc"
#undef RDYN_VJP_EXT
#undef RDYN_VJP_PARAMS
}

// What a link hook makes of its arguments: g = -(Y' w) of the link, the ten entries in the order of rdyn_nominal_parameters.  w' tau is
// the power of the link wrenches f = m d + alpha x h + omega x (omega x h), n = I alpha + omega x I omega + h x d (link_wrench) on the
// twists (ov, vv), so with d = acc + omega x v and e = ov x omega
//     d/dm = vv . d      d/dh = vv x alpha + omega x (omega x vv) + d x ov      d/dI = the six entries of sym(ov alpha' + e omega')
__device__ __forceinline__ void link_parameter_row(V3 om, V3 vl, V3 al, V3 acc, V3 ov, V3 vv, double (&g)[10])
{
  const V3 d = acc + cross(om, vl);
  const V3 e = cross(ov, om);
  const V3 gh = cross(vv, al) + cross(om, cross(om, vv)) + cross(d, ov);
  g[0] = -dot(vv, d);
  g[1] = -gh.x;
  g[2] = -gh.y;
  g[3] = -gh.z;
  g[4] = -fma(ov.x, al.x, e.x * om.x);
  g[5] = -(fma(ov.x, al.y, ov.y * al.x) + fma(e.x, om.y, e.y * om.x));
  g[6] = -(fma(ov.x, al.z, ov.z * al.x) + fma(e.x, om.z, e.z * om.x));
  g[7] = -fma(ov.y, al.y, e.y * om.y);
  g[8] = -(fma(ov.y, al.z, ov.z * al.y) + fma(e.y, om.z, e.z * om.y));
  g[9] = -fma(ov.z, al.z, e.z * om.z);
}

// ... and of the components: x[k * ld] += -row_k w_j for every column k of the list, in column order -- row the regressor row of the
// component (rdyn_component_row.h) at q / dq of its joint j, w by chain joint.  q, dq by chain joint as well.
template <int NJ>
__device__ __forceinline__ void component_parameter_rows(ChainPtr c, const RdynComponentTable& tb, const double (&q)[NJ], const double (&dq)[NJ],
                                                         const double (&w)[NJ], double* x, int64_t ld)
{
  int col = 0;
#pragma unroll 1
  for (int i = 0; i < tb.n_comps; ++i)
  {
    const RdynComponent& cp = tb.comps[i];
    double wj = 0.0, qj = 0.0, dqj = 0.0;
#pragma unroll
    for (int f = 0; f < NJ; ++f)
      if (c->j[f].in_idx == cp.joint)
      {
        wj = w[f];
        qj = q[f];
        dqj = dq[f];
      }
    double row[3];
    const int nc = component_row(cp, cp.type == RDYN_COMP_SPRING ? qj : dqj, row);
    for (int k = 0; k < nc; ++k, ++col) x[col * ld] += -(row[k] * wj);
  }
}
}  // namespace
#endif
