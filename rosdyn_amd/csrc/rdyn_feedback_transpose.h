// rdyn_feedback_transpose.h -- the transpose of the joint-space PD law (rdyn_feedback_law.h) as the adjoint kernels of the closed loop
// apply it: k_rollout_adjoint_fb (rdyn_rollout_adjoint_fb.hip) and k_rollout_adjoint_fb_params (rdyn_rollout_adjoint_fb_params.hip) share
// this text, as the forward kernels and the adjoint share fb_law.  The head of rdyn_rollout_adjoint_fb.hip has the scheme.
#ifndef RDYN_FEEDBACK_TRANSPOSE_H
#define RDYN_FEEDBACK_TRANSPOSE_H
#include <hip/hip_runtime.h>
#include "rdyn_rollout_adjoint_body.h"
#include "rdyn_feedback_law.h"

namespace
{
// The transpose of the law at one evaluation of the lane's sample in step t, at the state (q, dq) the command was formed at, by chain joint.
// ff = the step's feed-forward torques; tb = tot on entry, g on return; qb, vb = what the correction is applied to.  Returns false when
// a reference, a gain or a limit the sample reads is not finite.
template <int NJ, bool PER_SAMPLE>
__device__ __forceinline__ bool fb_transpose_gains(ChainPtr c, const RdynFeedbackArgs& fb, const RdynFeedbackGradArgs& gf, int64_t off, int64_t sj,
                                                   int t, const double (&ff)[NJ], const double (&q)[NJ], const double (&dq)[NJ], double (&tb)[NJ],
                                                   double (&qb)[NJ], double (&vb)[NJ])
{
  const bool vel = fb.kd != nullptr, clamp = fb.lim != nullptr;
  const int64_t at = (int64_t)t * fb.ref_step + off;
  uint64_t r0 = (uint64_t)(fb.q_ref + at), r1 = (uint64_t)(fb.dq_ref ? fb.dq_ref + at : nullptr);
  uint64_t g0 = (uint64_t)fb.kp, g1 = (uint64_t)fb.kd, g2 = (uint64_t)fb.lim;
  asm volatile("" : "+v"(r0), "+v"(r1));
  asm volatile("" : "+s"(g0), "+s"(g1), "+s"(g2));
  const double *const qr = (const double*)r0, *const dqr = (const double*)r1;
  const double *const kp = (const double*)g0, *const kd = (const double*)g1, *const lim = (const double*)g2;
  double* const gkp = gf.gkp ? gf.gkp + off : nullptr;
  double* const gkd = (vel && gf.gkd) ? gf.gkd + off : nullptr;
  double* const glim = (clamp && gf.glim) ? gf.glim + off : nullptr;
  bool ok = true;
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    const int idx = c->j[f].in_idx;
    if (idx < 0) continue;
    const int64_t o = idx * sj;
    const int64_t g = PER_SAMPLE ? off + o : (int64_t)idx;
    const double q_ref = qr[o], dq_ref = (vel && dqr) ? dqr[o] : 0.0;
    const double kpj = kp[g], kdj = vel ? kd[g] : 0.0, lm = clamp ? lim[idx] : 0.0;
    ok = ok && vjp_finite(q_ref) && vjp_finite(dq_ref) && vjp_finite(kpj) && vjp_finite(kdj) && vjp_finite(lm);
    const double u_raw = fb_law(ff[f], q_ref, q[f], kpj, vel, dq_ref, dq[f], kdj, false, 0.0);
    const bool hi = clamp && u_raw > lm, lo = clamp && !hi && u_raw < -lm;
    const double tot = tb[f];
    const double gj = (hi || lo) ? 0.0 : tot;
    qb[f] = fma(-kpj, gj, qb[f]);
    if (vel) vb[f] = fma(-kdj, gj, vb[f]);
    tb[f] = gj;
    if (gkp) gkp[o] = fma(q_ref - q[f], gj, gkp[o]);
    if (gkd) gkd[o] = fma(dq_ref - dq[f], gj, gkd[o]);
    if (glim) glim[o] += hi ? tot : (lo ? -tot : 0.0);
  }
  return ok;
}

// ... with the seed on the step's command record joined first (with_gu: the step's first evaluation)
template <int NJ>
__device__ __forceinline__ bool fb_transpose(ChainPtr c, const RdynFeedbackArgs& fb, const RdynFeedbackGradArgs& gf, int64_t off, int64_t sj, int t,
                                             bool with_gu, const double (&ff)[NJ], const double (&q)[NJ], const double (&dq)[NJ], double (&tb)[NJ],
                                             double (&qb)[NJ], double (&vb)[NJ])
{
  if (with_gu && gf.gu)  // wave-uniform
  {
    double gu[NJ];
    load_record<NJ>(c, gf.gu + (int64_t)t * gf.gu_step + off, sj, gu);
#pragma unroll
    for (int f = 0; f < NJ; ++f) tb[f] += gu[f];
  }
  if (fb.per_sample)  // wave-uniform
    return fb_transpose_gains<NJ, true>(c, fb, gf, off, sj, t, ff, q, dq, tb, qb, vb);
  return fb_transpose_gains<NJ, false>(c, fb, gf, off, sj, t, ff, q, dq, tb, qb, vb);
}

// the lane's rows of the sums (gkp, gkd, glim, and gq_ref / gdq_ref where they are one record): v to every entry -- 0.0 at the start of a
// call that does not continue earlier additions, quiet NaN at the end for a sample that failed
template <int NJ>
__device__ __forceinline__ void fb_rows_fill(ChainPtr c, const RdynFeedbackGradArgs& gf, int64_t off, int64_t sj, double v)
{
  double* const rows[5] = {gf.gkp, gf.gkd, gf.glim, gf.gref_step ? nullptr : gf.gq_ref, gf.gref_step ? nullptr : gf.gdq_ref};
#pragma unroll
  for (int r = 0; r < 5; ++r)
  {
    if (!rows[r]) continue;  // wave-uniform
#pragma unroll
    for (int f = 0; f < NJ; ++f)
    {
      const int idx = c->j[f].in_idx;
      if (idx >= 0) rows[r][off + idx * sj] = v;
    }
  }
}

// the reference gradients of step t once its gtau (gt; NaN for a sample that is no longer alive) is complete: kp * gt and kd * gt, to the
// step's records (through the wave's tile like gtau) or, with gref_step = 0, added to the lane's own record of the sums
template <int NJ>
__device__ __forceinline__ void fb_reference_gradients(ChainPtr c, const RdynFeedbackArgs& fb, const RdynFeedbackGradArgs& gf, const SmallRecords& sm,
                                                       bool stg, int64_t off, int64_t wave_off, int64_t sj, int t, const double (&gt)[NJ], int lane)
{
  double* const outs[2] = {gf.gq_ref, fb.kd ? gf.gdq_ref : nullptr};
  const double* const gains[2] = {fb.kp, fb.kd};
#pragma unroll
  for (int r = 0; r < 2; ++r)
  {
    if (!outs[r]) continue;  // wave-uniform
    uint64_t g0 = (uint64_t)gains[r];
    if (fb.per_sample)
      asm volatile("" : "+v"(g0));
    else
      asm volatile("" : "+s"(g0));
    const double* const gain = (const double*)g0;
    double v[NJ];
#pragma unroll
    for (int f = 0; f < NJ; ++f)
    {
      const int idx = c->j[f].in_idx;
      v[f] = idx >= 0 ? gain[fb.per_sample ? off + idx * sj : (int64_t)idx] * gt[f] : 0.0;
    }
    if (gf.gref_step)
    {
      const int64_t go = (int64_t)t * gf.gref_step;
      put_record<NJ>(c, sm, stg, v, outs[r] + go + wave_off, outs[r] + go + off, sj, lane);
    }
    else
    {
#pragma unroll
      for (int f = 0; f < NJ; ++f)
      {
        const int idx = c->j[f].in_idx;
        if (idx >= 0) outs[r][off + idx * sj] += v[f];
      }
    }
  }
}
}  // namespace
#endif
