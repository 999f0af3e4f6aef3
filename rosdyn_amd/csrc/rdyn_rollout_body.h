// rdyn_rollout_body.h -- what k_rollout (rdyn_rollout.hip) and its variant with components (rdyn_rollout_comp.hip) share besides the
// kernel text of rdyn_rollout_body.inc.
#ifndef RDYN_ROLLOUT_BODY_H
#define RDYN_ROLLOUT_BODY_H
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_record_stage.h"
#include "rdyn_fwd_dyn_body.h"

namespace
{
// one record (n_active doubles per sample, by input index) of the lane's sample: through the wave's tile, or from the lane
template <int NJ>
__device__ __forceinline__ void put_record(ChainPtr c, const SmallRecords& sm, bool stg, const double (&v)[NJ], double* wave_records, double* own,
                                           int64_t sj, int lane)
{
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    const int idx = c->j[f].in_idx;
    if (idx < 0) continue;
    if (stg) sm.put(idx, v[f]);
    else own[idx * sj] = v[f];
  }
  if (stg) sm.copy_out(wave_records, lane);
}

// The chain constants are loop-invariant, and so is every uniform double computed from them alone (sums of link parameters, products of
// axes): left to itself the optimiser hoists them out of the step loop and keeps them in vector registers across the whole evaluation
// (k_rollout<6, Euler>: 412 registers and scratch, against 257 of k_fwd_dyn<6>).  The pointer is laundered once per evaluation, so each
// evaluation reads its constants by scalar loads where it uses them, as k_fwd_dyn does.
__device__ __forceinline__ ChainPtr per_evaluation(ChainPtr c)
{
  uint64_t p = (uint64_t)c;
  asm volatile("" : "+s"(p));
  return (ChainPtr)p;
}
}  // namespace
#endif
