// rdyn_feedback_law.h -- the joint-space PD law of the closed-loop rollouts, the ONE text of it: k_rollout_fb and k_rollout_command
// (rdyn_rollout_fb.hip) form the command with it, and k_rollout_adjoint_fb (rdyn_rollout_adjoint_fb.hip) forms it again in the backward
// sweep, so the command the transpose is taken at carries the bits of the command the forward call applied.
#ifndef RDYN_FEEDBACK_LAW_H
#define RDYN_FEEDBACK_LAW_H
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_kernels.h"

namespace
{
// u = the law's command: u holds the feed-forward torques on entry.  One term of the law; both routes use this text.
__device__ __forceinline__ double fb_law(double ff, double q_ref, double q, double kp, bool vel, double dq_ref, double dq, double kd, bool clamp,
                                         double lim)
{
  double u = fma(kp, q_ref - q, ff);
  if (vel) u = fma(kd, dq_ref - dq, u);
  if (clamp) u = u > lim ? lim : (u < -lim ? -lim : u);
  return u;
}

// the command of the lane's sample at step t and state (q, dq), by chain joint: u[f] holds tau_ff on entry.  off = the sample's offset
// in an array addressed like q (s * in_ss), sj the stride between its joints.
// PER_SAMPLE: the gains are the lane's own (vector loads); otherwise indexed by the wave-uniform input index (scalar loads).
template <int NJ, bool PER_SAMPLE>
__device__ __forceinline__ void fb_command_gains(ChainPtr c, const RdynFeedbackArgs& fb, int64_t off, int64_t sj, int t, const double (&q)[NJ],
                                                 const double (&dq)[NJ], double (&u)[NJ])
{
  const bool vel = fb.kd != nullptr, clamp = fb.lim != nullptr;
  const int64_t at = (int64_t)t * fb.ref_step + off;
  uint64_t r0 = (uint64_t)(fb.q_ref + at), r1 = (uint64_t)(fb.dq_ref ? fb.dq_ref + at : nullptr);
  uint64_t g0 = (uint64_t)fb.kp, g1 = (uint64_t)fb.kd, g2 = (uint64_t)fb.lim;
  asm volatile("" : "+v"(r0), "+v"(r1));
  asm volatile("" : "+s"(g0), "+s"(g1), "+s"(g2));
  const double *const qr = (const double*)r0, *const dqr = (const double*)r1;
  const double *const kp = (const double*)g0, *const kd = (const double*)g1, *const lim = (const double*)g2;
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    const int idx = c->j[f].in_idx;
    if (idx < 0) continue;
    const int64_t o = idx * sj;
    const int64_t g = PER_SAMPLE ? off + o : (int64_t)idx;
    const double dr = (vel && dqr) ? dqr[o] : 0.0;
    u[f] = fb_law(u[f], qr[o], q[f], kp[g], vel, dr, dq[f], vel ? kd[g] : 0.0, clamp, clamp ? lim[idx] : 0.0);
  }
}

template <int NJ>
__device__ __forceinline__ void fb_command(ChainPtr c, const RdynFeedbackArgs& fb, int64_t off, int64_t sj, int t, const double (&q)[NJ],
                                           const double (&dq)[NJ], double (&u)[NJ])
{
  if (fb.per_sample)  // wave-uniform
    fb_command_gains<NJ, true>(c, fb, off, sj, t, q, dq, u);
  else
    fb_command_gains<NJ, false>(c, fb, off, sj, t, q, dq, u);
}
}  // namespace
#endif
