// rdyn_fwd_dyn_kernel.inc -- the body of k_fwd_dyn (rdyn_fwd_dyn.hip), included as text by the kernel and by its variant with components
// (rdyn_fwd_dyn_comp.hip), so that the plain kernel compiles to exactly what it was.  Expects: template parameter NJ; RdynFwdDynArgs a;
// RDYN_FWD_KERNEL_RHS(rhs): statements run once the torques are in rhs[NJ] (by chain joint), with c, qp, dqp and a in scope -- nothing in
// the plain kernel, rhs -= tau_c with components; RDYN_FWD_LINK_WRENCH: the hook of rdyn_fwd_dyn_body.inc, empty but with external wrenches.
  ChainPtr c = as_const(a.chain);
  const int lane = threadIdx.x;
  const int64_t s_wave = (int64_t)blockIdx.x * 64;
  const int64_t s = s_wave + lane;
  if (s >= a.n_samples) return;
  const bool stg = a.staged && a.n_samples - s_wave >= 64;  // wave-uniform: a full wave's records leave in whole lines
  const double* __restrict__ qp = a.q + s * a.in_ss;
  const double* __restrict__ dqp = a.dq + s * a.in_ss;
  const double* tp = a.tau + s * a.in_ss;  // (may alias ddq: every entry is read before the first store)

  double rhs[NJ];
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    const int idx = c->j[f].in_idx;
    rhs[f] = idx >= 0 ? tp[idx * a.in_sj] : 0.0;
  }

  RDYN_FWD_KERNEL_RHS(rhs)

#define RDYN_FWD_Q(f, idx) qp[idx * a.in_sj]
#define RDYN_FWD_DQ(f, idx) dqp[idx * a.in_sj]
#include "rdyn_fwd_dyn_body.inc"
#undef RDYN_FWD_Q
#undef RDYN_FWD_DQ

  if (a.status) a.status[s] = ok ? 1 : -1;
  const double qnan = __builtin_nan("");
  SmallRecords sm;
  if (stg)
  {
    extern __shared__ __attribute__((aligned(16))) char fwd_stage_lds[];
    sm.init(fwd_stage_lds, c->n_active, lane);
  }
  double* const op = a.ddq + s * a.in_ss;
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    const int idx = c->j[f].in_idx;
    if (idx < 0) continue;
    const double v = ok ? rhs[f] : qnan;
    if (stg) sm.put(idx, v);
    else op[idx * a.in_sj] = v;
  }
  if (stg) sm.copy_out(a.ddq + s_wave * a.in_ss, lane);
