// rdyn_component_row.h -- the regressor row of one additive component (friction, spring) and the component torque of a chain swept in
// registers.  component_row is what k_components (rdyn_components.hip) writes and what the forward dynamics and rollouts with components
// (rdyn_fwd_dyn_comp.hip, rdyn_rollout_comp.hip, k_fwd_solve's variant in rdyn_fwd_dyn.hip) subtract from the joint torque: one text, so the two agree bit for bit.
// component_slope is its derivative, which the derivatives of the forward dynamics (rdyn_fwd_dyn_deriv.hip) put on the diagonals.
#ifndef RDYN_COMPONENT_ROW_H
#define RDYN_COMPONENT_ROW_H
#include <hip/hip_runtime.h>
#include "rdyn_kernels.h"

namespace
{
// row of component c at x = q of its joint (RDYN_COMP_SPRING) or Dq of its joint (friction); returns the number of columns
__device__ __forceinline__ int component_row(const RdynComponent& c, double x, double (&row)[3])
{
  row[2] = 0.0;
  if (c.type == RDYN_COMP_SPRING)
  {
    row[0] = x;
    row[1] = 1.0;
    return 2;
  }
  const double omega = fmin(fmax(x, -c.max_velocity), c.max_velocity);
  double sg;
  if (c.type == RDYN_COMP_FRICTION1)
    sg = fmin(fmax(omega / c.min_velocity, -1.0), 1.0);
  else
    sg = (omega == 0.0) ? 0.0 : (omega > c.min_velocity ? 1.0 : (omega < -c.min_velocity ? -1.0 : omega / c.min_velocity));
  row[0] = sg;
  row[1] = omega;
  row[2] = omega * omega * sg;
  return c.type == RDYN_COMP_FRICTION2 ? 3 : 2;
}

// row . parameters, accumulated as k_components accumulates it
__device__ __forceinline__ double component_torque(const RdynComponent& c, double x)
{
  double row[3];
  const int cols = component_row(c, x, row);
  double t = 0.0;
  for (int k = 0; k < cols; ++k) t = fma(row[k], c.parameters[k], t);
  return t;
}

// d (row . parameters) / d x of component c at x: the slope of component_torque in its own argument (q of the joint for a spring, Dq for
// friction).  With omega = clamp(x, +-max_velocity) and sg the saturated sign of component_row: omega' = 1 for |x| < max_velocity, else
// 0; sg' = 1 / min_velocity for |omega| < min_velocity, else 0.  EXACTLY AT A KINK (|x| = max_velocity, |omega| = min_velocity) this is
// the OUTER one-sided slope: the one of the saturated side.
__device__ __forceinline__ double component_slope(const RdynComponent& c, double x)
{
  if (c.type == RDYN_COMP_SPRING) return c.parameters[0];
  if (!(fabs(x) < c.max_velocity)) return 0.0;
  const double omega = x;  // (not clamped here)
  const bool band = fabs(omega) < c.min_velocity;
  const double dsg = band ? 1.0 / c.min_velocity : 0.0;
  double s = fma(c.parameters[0], dsg, c.parameters[1]);
  if (c.type == RDYN_COMP_FRICTION2)
  {
    const double sg = band ? omega / c.min_velocity : (omega > 0.0 ? 1.0 : -1.0);
    s = fma(c.parameters[2], fma(2.0 * omega, sg, omega * omega * dsg), s);
  }
  return s;
}

// d tau_c / d q (kind 0: the springs) or d tau_c / d Dq (kind 1: the friction components) of input joint idx, the components of that
// joint in list order
__device__ __forceinline__ double joint_component_slope(const RdynComponentTable& t, int idx, int kind, double qv, double dqv)
{
  double sl = 0.0;
#pragma unroll 1
  for (int i = 0; i < t.n_comps; ++i)
  {
    const RdynComponent& c = t.comps[i];
    if (c.joint != idx || (c.type == RDYN_COMP_SPRING) != (kind == 0)) continue;
    sl += component_slope(c, kind == 0 ? qv : dqv);
  }
  return sl;
}

// tau_c of input joint idx at (qv, dqv): the components of that joint in list order, summed as k_components sums them into a
// zero-initialised tau_add.  The loop over the list is wave-uniform (the table sits in the kernel arguments) and has a run-time trip
// count: every constant of a component is read by scalar loads where it is used, nothing of the table is kept in vector registers.
__device__ __forceinline__ double joint_component_torque(const RdynComponentTable& t, int idx, double qv, double dqv)
{
  double tc = 0.0;
#pragma unroll 1
  for (int i = 0; i < t.n_comps; ++i)
  {
    const RdynComponent& c = t.comps[i];
    if (c.joint != idx) continue;
    tc += component_torque(c, c.type == RDYN_COMP_SPRING ? qv : dqv);
  }
  return tc;
}
}  // namespace
#endif
