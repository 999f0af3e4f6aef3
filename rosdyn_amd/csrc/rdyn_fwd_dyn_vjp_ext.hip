// rdyn_fwd_dyn_vjp_ext.hip -- batched reverse-mode products of the forward dynamics with external link wrenches
// (rdyn_forward_dynamics_vjp_ext; no counterpart in the reference): with ddq = FD_E(q, dq, tau, ext) = FD_c(q, dq, tau - tau_E(q, ext)),
// a seed ddq_bar per sample and w = M^-1 ddq_bar
//     tau_bar = w,   dq_bar as in rdyn_forward_dynamics_vjp,   q_bar = -(dtau_dq + diag d tau_c / d q + d tau_E / d q)' w,
//     ext_bar = -(d tau_E / d ext)' w,
// tau_E the joint torque of the wrenches alone in the convention of rdyn_joint_torque_ext (rdyn_ext_wrench.h).
//   k_fwd_dyn_vjp_ext<NJ>   k_fwd_dyn_vjp with the third form of the product (fwd_dyn_vjp_ext_eval, rdyn_fwd_dyn_vjp_body.h): still ONE
//     launch.  The wrenches are read where their link is swept (every link: 6 doubles per link and sweep, 3 per link and KIND 0 column;
//     one link: 6 doubles per lane, loaded with the torques); ext_bar leaves where its link is swept, 6 doubles per link, nothing carried.
//     The base link's record is +0.0.  A translation unit of its own: it builds beside rdyn_fwd_dyn_vjp.hip, whose code object stays what
//     it was.
// A sample whose factorisation failed the pivot rule, or with a non-finite state, torque, seed or wrench entry it reads, gets status -1
// and quiet NaN in every output.
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_record_stage.h"
#include "rdyn_rollout_body.h"
#include "rdyn_fwd_dyn_vjp_body.h"
#include "rdyn_ext_wrench.h"
#include "rdyn_launch_util.h"

namespace
{
template <int NJ>
__global__ __launch_bounds__(64) void k_fwd_dyn_vjp_ext(const RdynFwdDynVjpExtArgs ax)
{
  const RdynFwdDynVjpArgs& a = ax.v;
  ChainPtr c = as_const(a.chain);
  const int lane = threadIdx.x;
  const int64_t s_wave = (int64_t)blockIdx.x * 64;
  const int64_t s = s_wave + lane;
  if (s >= a.n_samples) return;
  const bool stg = a.staged && a.n_samples - s_wave >= 64;  // wave-uniform: a full wave's records leave in whole lines

  const double* __restrict__ qp = a.q + s * a.in_ss;
  const double* __restrict__ dqp = a.dq + s * a.in_ss;
  double rhs[NJ], ab[NJ], qb[NJ], vb[NJ];
  ExtEval xe;
  xe.rec = ax.x.w + s * ax.x.ss;
  xe.se = ax.x.se;
  xe.one = ax.x.one;
  xe.l = xe.a = mk(0, 0, 0);
  {
    const double* __restrict__ tp = a.tau + s * a.in_ss;
    const double* sp = a.ddq_bar + s * a.in_ss;  // (may alias tau_bar: every entry is read before the first store)
#pragma unroll
    for (int f = 0; f < NJ; ++f)
    {
      const int idx = c->j[f].in_idx;
      rhs[f] = idx >= 0 ? tp[idx * a.in_sj] : 0.0;
      ab[f] = idx >= 0 ? sp[idx * a.in_sj] : 0.0;
    }
    if (xe.one) ext_load6(xe.rec, xe.se, xe.l, xe.a);
  }
  SmallRecords sm;
  if (stg)
  {
    extern __shared__ __attribute__((aligned(16))) char vjp_ext_stage_lds[];
    sm.init(vjp_ext_stage_lds, c->n_active, lane);
  }
  const double qnan = __builtin_nan("");
  const int64_t ow = s_wave * a.in_ss, oo = s * a.in_ss;
  double* const eb = ax.ext_bar ? ax.ext_bar + s * ax.x.ss : nullptr;
  const int64_t se = ax.x.se;
  const int one = ax.x.one;
  bool use = false;  // the verdict, known behind early()
  const bool ok = fwd_dyn_vjp_ext_eval<NJ>(
      c, a.t, [&](int, int idx) { return qp[idx * a.in_sj]; }, [&](int, int idx) { return dqp[idx * a.in_sj]; }, rhs, ab, qb, vb,
      a.q_bar != nullptr, a.dq_bar != nullptr,
      [&](bool good, double (&ddq)[NJ]) {
        use = good;
        if (a.status) a.status[s] = good ? 1 : -1;
        if (eb && one <= 1)
        {
          // the base link's record: +0.0 (every link: the first of the records; one link: the record when the link is the base)
          const double z = good ? 0.0 : qnan;
#pragma unroll
          for (int e = 0; e < 6; ++e) eb[e * se] = z;
        }
        if (!a.ddq) return;  // wave-uniform
        double v[NJ];
#pragma unroll
        for (int f = 0; f < NJ; ++f) v[f] = good ? ddq[f] : qnan;
        put_record<NJ>(c, sm, stg, v, a.ddq + ow, a.ddq + oo, a.in_sj, lane);
      },
      xe, eb != nullptr,
      [&](int link, V3 lin, V3 ang) {
        if (one != 0 && one != link + 1) return;  // wave-uniform
        double* const p = eb + (one ? 0 : (int64_t)(6 * link) * se);
        p[0] = use ? lin.x : qnan;
        p[se] = use ? lin.y : qnan;
        p[2 * se] = use ? lin.z : qnan;
        p[3 * se] = use ? ang.x : qnan;
        p[4 * se] = use ? ang.y : qnan;
        p[5 * se] = use ? ang.z : qnan;
      });
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    ab[f] = ok ? ab[f] : qnan;
    qb[f] = ok ? qb[f] : qnan;
    vb[f] = ok ? vb[f] : qnan;
  }
  if (a.tau_bar) put_record<NJ>(c, sm, stg, ab, a.tau_bar + ow, a.tau_bar + oo, a.in_sj, lane);
  if (a.q_bar) put_record<NJ>(c, sm, stg, qb, a.q_bar + ow, a.q_bar + oo, a.in_sj, lane);
  if (a.dq_bar) put_record<NJ>(c, sm, stg, vb, a.dq_bar + ow, a.dq_bar + oo, a.in_sj, lane);
}

template <int NJ>
hipError_t launch_vjp_ext_nj(const RdynFwdDynVjpExtArgs& a, hipStream_t st)
{
  const size_t lds = a.v.staged ? (size_t)64 * (size_t)(a.v.staged | 1) * 8 : 0;
  hipLaunchKernelGGL((k_fwd_dyn_vjp_ext<NJ>), dim3((unsigned)((a.v.n_samples + 63) / 64)), dim3(64), lds, st, a);
  return hipGetLastError();
}
}  // namespace

hipError_t rdyn_launch_forward_dynamics_vjp_ext(int n_joints, const RdynFwdDynVjpExtArgs& a, hipStream_t st)
{
  if (a.v.n_samples <= 0) return hipSuccess;
  if (a.v.t.n_comps < 0 || a.v.t.n_comps > RDYN_MAX_COMPONENTS || (!a.v.q_bar && !a.v.dq_bar && !a.v.tau_bar && !a.ext_bar))
    return hipErrorInvalidValue;
  if (!a.x.w || a.x.one < 0 || a.x.one > n_joints + 1) return hipErrorInvalidValue;
#define CALL(N) launch_vjp_ext_nj<N>(a, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}
