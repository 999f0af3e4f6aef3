// rdyn_ext_wrench.h -- external link wrenches inside one forward-dynamics evaluation (k_fwd_dyn_ext, rdyn_fwd_dyn_ext.hip; k_rollout_ext,
// rdyn_rollout_ext.hip).  A wrench [force; torque] applied TO chain link l, given in the link's own frame, enters the link's net wrench
// with the reference's sign and transform (getWrench, primitives_impl.h:1255: spatialTranformation(-ext, T_bl), the TWIST-form transform
// with the link's absolute position, reproduced as it is): in link coordinates [-(e.lin + e.ang x R_l^T p_l) ; -e.ang], the statement of
// rdyn_local_sweep_body.inc's torque mode.  The forward sweep of rdyn_fwd_dyn_body.inc has each link's frame; its hook
// RDYN_FWD_LINK_WRENCH calls ext_link_wrench, which carries the link origin in link coordinates (pl) and subtracts the contribution from
// (Fo[f], No[f]) before the backward pass -- no second kinematic sweep, no tau_E vector.  The base link's record never enters.
#ifndef RDYN_EXT_WRENCH_H
#define RDYN_EXT_WRENCH_H
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_fwd_dyn_body.h"

namespace
{
// the wrenches one evaluation sees: every link's record in memory (one = 0: read where the link is swept, 6 doubles at a time, nothing
// carried), or one link's wrench in registers (one = 1 + link)
struct ExtEval
{
  const double* rec;  // the lane's links x 6 record of the step, element e at rec[e * se]
  int64_t se;
  int one;
  V3 l, a;
};

__device__ __forceinline__ void ext_load6(const double* p, int64_t se, V3& l, V3& a)
{
  l = mk(p[0], p[se], p[2 * se]);
  a = mk(p[3 * se], p[4 * se], p[5 * se]);
}

// link = f + 1, R, t = the transform of joint f; pl: the origin of link f in its coordinates on entry, of link f + 1 on return
__device__ __forceinline__ void ext_link_wrench(const ExtEval& x, int link, const double* R, V3 t, V3& pl, V3& fo, V3& no)
{
  pl = rotT(R, pl + t);
  V3 el, ea;
  if (x.one == 0)
    ext_load6(x.rec + (int64_t)(6 * link) * x.se, x.se, el, ea);
  else if (x.one == link + 1)
  {
    el = x.l;
    ea = x.a;
  }
  else
    return;
  fo = fo - (el + cross(ea, pl));
  no = no - ea;
}

// the evaluation of rdyn_fwd_dyn_body.h at a state held in registers, with the wrenches of x: returns ok.  The record pointer is laundered
// once per evaluation: the loads of the all-link mode are loop-invariant over RK4's stages, and hoisted out of the stage loop they would
// live in 12 (NJ + 1) registers across the evaluations (the per_evaluation concern of rdyn_rollout_body.h).
template <int NJ>
__device__ __forceinline__ bool fwd_dyn_eval_ext(ChainPtr c, const double (&q)[NJ], const double (&dq)[NJ], double (&rhs)[NJ], ExtEval x)
{
  {
    uint64_t p = (uint64_t)x.rec;
    asm volatile("" : "+v"(p));
    x.rec = (const double*)p;
  }
  V3 pl = mk(0, 0, 0);
#define RDYN_FWD_Q(f, idx) q[f]
#define RDYN_FWD_DQ(f, idx) dq[f]
#define RDYN_FWD_LINK_WRENCH(f, R, t, fo, no) ext_link_wrench(x, f + 1, R, t, pl, fo, no);
#include "rdyn_fwd_dyn_body.inc"
#undef RDYN_FWD_LINK_WRENCH
#undef RDYN_FWD_Q
#undef RDYN_FWD_DQ
  return ok;
}
}  // namespace
#endif
