// rdyn_rotvec.h -- the rotation part of getFrameDistance (frame_distance.h:44-49), shared by the local IK kernels
// (rdyn_ik.hip, rdyn_long_ik.hip) and k_frame_distance.
#ifndef RDYN_ROTVEC_H
#define RDYN_ROTVEC_H
#include <hip/hip_runtime.h>
#include "rdyn_devmath.h"

namespace
{

// Eigen::Quaterniond(R) (Eigen 3.3/3.4: trace / largest-diagonal branches), R row-major
__device__ __forceinline__ void quaternion_of(const double (&M)[9], double& qx, double& qy, double& qz, double& qw)
{
  double t = M[0] + M[4] + M[8];
  if (t > 0.0)
  {
    t = sqrt(t + 1.0);
    qw = 0.5 * t;
    t = 0.5 / t;
    qx = (M[7] - M[5]) * t;
    qy = (M[2] - M[6]) * t;
    qz = (M[3] - M[1]) * t;
  }
  else if (M[0] >= M[4] && M[0] >= M[8])  // i = 0
  {
    t = sqrt(M[0] - M[4] - M[8] + 1.0);
    qx = 0.5 * t;
    t = 0.5 / t;
    qw = (M[7] - M[5]) * t;
    qy = (M[3] + M[1]) * t;
    qz = (M[6] + M[2]) * t;
  }
  else if (M[4] >= M[8])  // i = 1
  {
    t = sqrt(M[4] - M[8] - M[0] + 1.0);
    qy = 0.5 * t;
    t = 0.5 / t;
    qw = (M[2] - M[6]) * t;
    qz = (M[7] + M[5]) * t;
    qx = (M[1] + M[3]) * t;
  }
  else  // i = 2
  {
    t = sqrt(M[8] - M[0] - M[4] + 1.0);
    qz = 0.5 * t;
    t = 0.5 / t;
    qw = (M[3] - M[1]) * t;
    qx = (M[2] + M[6]) * t;
    qy = (M[5] + M[7]) * t;
  }
}

// Eigen::AngleAxisd(R).angle() * .axis()  (Eigen 3.3/3.4: quaternion -> angle in [0, pi], axis = sign(w) vec / |vec|)
__device__ __forceinline__ V3 rotation_vector(const double (&M)[9])
{
  double qx, qy, qz, qw;
  quaternion_of(M, qx, qy, qz, qw);
  const double n = sqrt(fma(qx, qx, fma(qy, qy, qz * qz)));
  if (n == 0.0) return mk(0, 0, 0);
  const double k = 2.0 * atan2(n, fabs(qw)) / (qw < 0.0 ? -n : n);
  return mk(qx * k, qy * k, qz * k);
}

}  // namespace

#endif
