// rdyn_joint_step.h -- device side: the steps of the local-frame recursions (velocity state down the chain, wrenches and composite bodies
// back up) that the forward dynamics (rdyn_fwd_dyn_body.h) and the torque derivatives (rdyn_torque_deriv.hip) share.
#ifndef RDYN_JOINT_STEP_H
#define RDYN_JOINT_STEP_H
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"

namespace
{
// what a sweep saves of a joint's position: sin q, 1 - cos q (revolute) or q, 0 (prismatic, fixed)
__device__ __forceinline__ void joint_sincos_state(int type, double qf, double& s0, double& s1)
{
  if (type == RDYN_REVOLUTE)
  {
    double sn, cs;
    rdyn_sincos(qf, &sn, &cs);
    s0 = sn;
    s1 = 1.0 - cs;
  }
  else
  {
    s0 = qf;
    s1 = 0.0;
  }
}

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

// the velocity state of a link carried into its child frame and the child joint's own motion added (rdyn_local_sweep_body.inc)
__device__ __forceinline__ void primal_step(JointRef J, const double (&R)[9], V3 t, double dqf, double ddqf, V3& w, V3& vl, V3& al, V3& acc)
{
  const V3 wn = rotT(R, w);
  const V3 vn = rotT(R, vl + cross(w, t));
  const V3 aln = rotT(R, al);
  const V3 an = rotT(R, acc + cross(al, t));
  w = wn; vl = vn; al = aln; acc = an;
  const V3 u = ld3(J.u);
  if (J.type == RDYN_REVOLUTE)
  {
    acc = axpy(acc, cross(vl, u), dqf);
    al = axpy(axpy(al, cross(w, u), dqf), u, ddqf);
    w = axpy(w, u, dqf);
  }
  else if (J.type == RDYN_PRISMATIC)
  {
    acc = axpy(axpy(acc, cross(w, u), dqf), u, ddqf);
    vl = axpy(vl, u, dqf);
  }
}

// net wrench of a link about its origin, own frame (getWrench, primitives_impl.h:1240-1250)
__device__ __forceinline__ void link_wrench(JointRef J, V3 w, V3 vl, V3 al, V3 acc, V3& fo, V3& no)
{
  const RDYN_CONST_AS double* pi = J.pi;
  const double m = pi[0];
  const V3 h = ld3(pi + 1);
  const V3 d = acc + cross(w, vl);
  fo = axpy(cross(al, h) + cross(w, cross(w, h)), d, m);
  no = symv(pi + 4, al) + cross(w, symv(pi + 4, w)) + cross(h, d);
}

// a composite body (m, h = m c, I about the origin) into the parent's frame, x_parent = R x + t: returns h' = R h + m t and leaves
// I' = R I R' + (m |t|^2 + 2 t.hb) 1 - (m t t' + t hb' + hb t'), hb = R h, in cI.  (h by value and returned: handed over by
// reference, two instantiations of k_torque_deriv came out one instruction longer.)
__device__ __forceinline__ V3 composite_to_parent(const double (&R)[9], V3 t, double cm, V3 ch, double (&cI)[6])
{
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
  return axpy(hb, t, cm);
}
}  // namespace
#endif
