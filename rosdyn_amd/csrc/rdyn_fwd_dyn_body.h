// rdyn_fwd_dyn_body.h -- one evaluation of the forward dynamics ddq = M(q)^-1 (tau - h(q, dq)) of a chain swept in registers, shared by
// k_fwd_dyn (rdyn_fwd_dyn.hip: one evaluation per sample) and k_rollout (rdyn_rollout.hip: one per integrator stage, the state staying
// in registers between them).  The three passes -- forward sweep, composite-rigid-body backward pass, Cholesky with both solves -- are
// described at the head of rdyn_fwd_dyn.hip and written once, in rdyn_fwd_dyn_body.inc.  k_fwd_dyn includes that text in place with q and
// dq loaded where they are used: called through the function below (any way of handing it the loads: a functor, a flag) its register
// figures moved (k_fwd_dyn<3> 166 -> 167 VGPRs, <9> and <10> 104 -> 98 and 146 -> 138 AGPRs), and the refactoring was not to change it.
// k_rollout calls the function, q and dq in registers.  The same holds for the steps of rdyn_joint_step.h: joint_transform and
// composite_to_parent are called (every kernel's registers, scratch and instruction count as before); joint_sincos_state moved the
// registers of k_fwd_dyn<8..10> (320 -> 318, 360 -> 358, 402 -> 406 VGPRs), link_wrench those of k_rollout<5..6, .> and the scratch of
// k_rollout<10, .> (0 -> 20 B with Euler), and the forward step with DDq = 0 is not primal_step (one more fma per axis): these three stay
// written out in the .inc.
#ifndef RDYN_FWD_DYN_BODY_H
#define RDYN_FWD_DYN_BODY_H
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_joint_step.h"

namespace
{
#define RDYN_FWD_PIVOT_FLOOR 1e-10  // rdyn_ik.hip's RDYN_IK_PIVOT_FLOOR
#define TRI(i, j) ((i) * ((i) + 1) / 2 + (j))  // lower triangle, i >= j

// the evaluation at a state held in registers (by chain joint): returns ok
template <int NJ>
__device__ __forceinline__ bool fwd_dyn_eval(ChainPtr c, const double (&q)[NJ], const double (&dq)[NJ], double (&rhs)[NJ])
{
#define RDYN_FWD_Q(f, idx) q[f]
#define RDYN_FWD_DQ(f, idx) dq[f]
#define RDYN_FWD_LINK_WRENCH(f, R, t, fo, no)
#include "rdyn_fwd_dyn_body.inc"
#undef RDYN_FWD_LINK_WRENCH
#undef RDYN_FWD_Q
#undef RDYN_FWD_DQ
  return ok;
}
}  // namespace
#endif
