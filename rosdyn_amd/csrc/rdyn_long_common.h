// rdyn_long_common.h -- device pieces shared by the rolled-loop kernels of chains with more input joints than the unrolled kernels sweep
// (rdyn_long_kin.hip, rdyn_long_local.hip, rdyn_long_ik.hip, k_long_torque_deriv): the chain constants' pointer, one step of the
// base-frame frame recursion and the wave-private per-joint state in LDS.
#ifndef RDYN_LONG_COMMON_H
#define RDYN_LONG_COMMON_H
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"

namespace
{
typedef const RDYN_CONST_AS RdynLongChainConst* LongChainPtr;
__device__ __forceinline__ LongChainPtr as_const_long(const RdynLongChainConst* p)
{
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
  return (LongChainPtr)p;
#pragma clang diagnostic pop
}

// One step of computeFrames / computeScrews (primitives_impl.h:863-882): on entry R, p = frame of the parent link; on exit of the
// child.  zl = the joint axis in the base frame (rotated by the PARENT frame, :879), d = p_child - p_parent.
__device__ __forceinline__ void frame_step(JointRef J, double qf, double (&R)[9], V3& p, V3& zl, V3& d)
{
  const int type = J.type;
  double Rpc[9];
  V3 t = ld3(J.t);
  if (type == RDYN_REVOLUTE)
  {
    double sn, cs;
    rdyn_sincos(qf, &sn, &cs);
    const double oc = 1.0 - cs;
#pragma unroll
    for (int i = 0; i < 9; ++i) Rpc[i] = fma(sn, J.B[i], fma(oc, J.C[i], J.A[i]));
  }
  else
  {
#pragma unroll
    for (int i = 0; i < 9; ++i) Rpc[i] = J.A[i];
    if (type == RDYN_PRISMATIC) t = axpy(t, ld3(J.up), qf);
  }
  zl = rot(R, ld3(J.up));
  d = rot(R, t);
  double Rn[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) Rn[r * 3 + cc] = fma(R[r * 3 + 0], Rpc[cc], fma(R[r * 3 + 1], Rpc[3 + cc], R[r * 3 + 2] * Rpc[6 + cc]));
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = Rn[i];
  p = p + d;
}

// wave-private per-joint state: value v of joint j of the lane's sample at st[(v * nj + j) * lanes + lane] (st = the area + lane; lanes =
// the lanes of the workgroup, 64 everywhere but in k_long_torque_deriv)
struct JointState
{
  double* st;
  int nj, lanes;
  __device__ __forceinline__ double& at(int v, int j) const { return st[(v * nj + j) * lanes]; }
  __device__ __forceinline__ void put3(int v0, int j, V3 x) const
  {
    at(v0, j) = x.x;
    at(v0 + 1, j) = x.y;
    at(v0 + 2, j) = x.z;
  }
  __device__ __forceinline__ V3 get3(int v0, int j) const { return mk(at(v0, j), at(v0 + 1, j), at(v0 + 2, j)); }
};
}  // namespace
#endif
