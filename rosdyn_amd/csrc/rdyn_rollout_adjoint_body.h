// rdyn_rollout_adjoint_body.h -- what k_rollout_adjoint (rdyn_rollout_adjoint.hip) and k_rollout_adjoint_params
// (rdyn_rollout_adjoint_params.hip) share beside the text of their body (rdyn_rollout_adjoint_body.inc).
#ifndef RDYN_ROLLOUT_ADJOINT_BODY_H
#define RDYN_ROLLOUT_ADJOINT_BODY_H
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_record_stage.h"
#include "rdyn_fwd_dyn_body.h"
#include "rdyn_rollout_body.h"
#include "rdyn_component_row.h"
#include "rdyn_fwd_dyn_vjp_body.h"

namespace
{
// where the lanes of k_rollout_adjoint_params accumulate
struct RdynAdjointParamAcc
{
  double* acc;       // [10 NJ + n_comp_cols][ld]: column k of sample s at acc[k * ld + s]
  int64_t ld;
  int32_t* status;   // [n_samples]: 1, or -1 for a sample that failed anywhere on the horizon
  int n_comp_cols;
};

template <int NJ>
__device__ __forceinline__ void load_record(ChainPtr c, const double* p, int64_t sj, double (&v)[NJ])
{
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    const int idx = c->j[f].in_idx;
    v[f] = (idx >= 0 && p) ? p[idx * sj] : 0.0;
  }
}
}  // namespace
#endif
