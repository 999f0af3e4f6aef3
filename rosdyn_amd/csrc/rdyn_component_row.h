// rdyn_component_row.h -- the regressor row of one additive component (friction, spring) and the component torque of a chain swept in
// registers.  component_row is what k_components (rdyn_components.hip) writes and what the forward dynamics and rollouts with components
// (rdyn_fwd_dyn_comp.hip, rdyn_rollout_comp.hip, k_fwd_solve's variant in rdyn_fwd_dyn.hip) subtract from the joint torque: one text, so the two agree bit for bit.
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
