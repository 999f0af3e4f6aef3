// rdyn_fwd_dyn_body.h -- one evaluation of the forward dynamics ddq = M(q)^-1 (tau - h(q, dq)) of a chain swept in registers, shared by
// k_fwd_dyn (rdyn_fwd_dyn.hip: one evaluation per sample) and k_rollout (rdyn_rollout.hip: one per integrator stage, the state staying
// in registers between them).  The three passes -- forward sweep, composite-rigid-body backward pass, Cholesky with both solves -- are
// described at the head of rdyn_fwd_dyn.hip and written once, in rdyn_fwd_dyn_body.inc.  k_fwd_dyn includes that text in place with q and
// dq loaded where they are used: called through the function below (any way of handing it the loads: a functor, a flag) its register
// figures moved (k_fwd_dyn<3> 166 -> 167 VGPRs, <9> and <10> 104 -> 98 and 146 -> 138 AGPRs), and the refactoring was not to change it.
// k_rollout calls the function, q and dq in registers.
#ifndef RDYN_FWD_DYN_BODY_H
#define RDYN_FWD_DYN_BODY_H
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"

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

// the evaluation at a state held in registers (by chain joint): returns ok
template <int NJ>
__device__ __forceinline__ bool fwd_dyn_eval(ChainPtr c, const double (&q)[NJ], const double (&dq)[NJ], double (&rhs)[NJ])
{
#define RDYN_FWD_Q(f, idx) q[f]
#define RDYN_FWD_DQ(f, idx) dq[f]
#include "rdyn_fwd_dyn_body.inc"
#undef RDYN_FWD_Q
#undef RDYN_FWD_DQ
  return ok;
}
}  // namespace
#endif
