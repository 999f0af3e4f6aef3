// rdyn_tangent_step.h -- device side: the forward-mode tangent of the local-frame recursion, one input joint at a time (the algorithm is
// described at the head of rdyn_torque_deriv.hip), shared by the derivatives of the inverse dynamics (rdyn_torque_deriv.hip) and of the
// forward dynamics (rdyn_fwd_dyn_deriv.hip).
#ifndef RDYN_TANGENT_STEP_H
#define RDYN_TANGENT_STEP_H
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_joint_step.h"

namespace
{
struct Tangent
{
  V3 w, vl, al, acc;
};

// the tangent state at link k for a unit change of q_k (KIND 0) or Dq_k (KIND 1)
__device__ __forceinline__ Tangent tangent_seed(int kind, int type, V3 u, V3 w, V3 vl, V3 al, V3 acc)
{
  Tangent d;
  const V3 z = mk(0, 0, 0);
  d.w = z; d.vl = z; d.al = z; d.acc = z;
  if (kind == 0)
  {
    if (type == RDYN_REVOLUTE)
    {
      d.w = cross(w, u);
      d.vl = cross(vl, u);
      d.al = cross(al, u);
      d.acc = cross(acc, u);
    }
    else if (type == RDYN_PRISMATIC)
    {
      d.vl = cross(w, u);
      d.acc = cross(al, u);
    }
  }
  else
  {
    if (type == RDYN_REVOLUTE)
    {
      d.w = u;
      d.al = cross(w, u);
      d.acc = cross(vl, u);
    }
    else if (type == RDYN_PRISMATIC)
    {
      d.vl = u;
      d.acc = cross(w, u);
    }
  }
  return d;
}

// the tangent state through a joint DOWNSTREAM of the differentiated one (its transform is a constant of the derivative)
__device__ __forceinline__ void tangent_step(JointRef J, const double (&R)[9], V3 t, double dqf, Tangent& d)
{
  const V3 wn = rotT(R, d.w);
  const V3 vn = rotT(R, d.vl + cross(d.w, t));
  const V3 aln = rotT(R, d.al);
  const V3 an = rotT(R, d.acc + cross(d.al, t));
  d.w = wn; d.vl = vn; d.al = aln; d.acc = an;
  const V3 u = ld3(J.u);
  if (J.type == RDYN_REVOLUTE)
  {
    d.acc = axpy(d.acc, cross(d.vl, u), dqf);
    d.al = axpy(d.al, cross(d.w, u), dqf);
  }
  else if (J.type == RDYN_PRISMATIC)
    d.acc = axpy(d.acc, cross(d.w, u), dqf);
}

// tangent of link_wrench at the primal (w, vl)
__device__ __forceinline__ void tangent_wrench(JointRef J, V3 w, V3 vl, const Tangent& d, V3& dfo, V3& dno)
{
  const RDYN_CONST_AS double* pi = J.pi;
  const double m = pi[0];
  const V3 h = ld3(pi + 1);
  const V3 dd = d.acc + cross(d.w, vl) + cross(w, d.vl);
  dfo = axpy(cross(d.al, h) + cross(d.w, cross(w, h)) + cross(w, cross(d.w, h)), dd, m);
  dno = symv(pi + 4, d.al) + cross(d.w, symv(pi + 4, w)) + cross(w, symv(pi + 4, d.w)) + cross(h, dd);
}
}  // namespace
#endif
