// rdyn_rollout_body.inc -- the body of k_rollout (rdyn_rollout.hip), included as text by the kernel and by its variant with components
// (rdyn_rollout_comp.hip), so that the plain kernel compiles to exactly what it was.  Expects: template parameters NJ, INTEGRATOR;
// RdynRolloutArgs a; RDYN_ROLLOUT_RHS(q, dq, rhs): statements run immediately before each evaluation, the stage state in q[NJ], dq[NJ] and
// the step's torques in rhs[NJ] (all by chain joint), with c in scope -- nothing in the plain kernel, rhs -= tau_c(q, dq) with components;
// RDYN_ROLLOUT_EVAL(c, q, dq, rhs): the evaluation, fwd_dyn_eval<NJ> but with external wrenches (rdyn_rollout_ext.hip), whose kernel also
// fills RDYN_ROLLOUT_TAKE (statements run where rhs takes its copy of the step's torques, the step t in scope: the step's wrench is taken
// the same way) and RDYN_ROLLOUT_PREFETCH (statements run where the torques of step t + 1 are requested); both empty everywhere else.
// RDYN_ROLLOUT_HEAD: optional, statements run at the head of step t, before its first evaluation, with the step's start state in q, dq,
// its torques in tau and alive, due, rec_off, sm, stg_traj in scope: the closed-loop kernel (rdyn_rollout_fb.hip) forms the held command
// into tau there and writes the command record that is due.  Empty unless the including kernel defines it.
#ifndef RDYN_ROLLOUT_HEAD
#define RDYN_ROLLOUT_HEAD
#define RDYN_ROLLOUT_HEAD_DEFAULTED
#endif
  const ChainPtr c = as_const(a.chain);
  const int lane = threadIdx.x;
  const int64_t s_wave = (int64_t)blockIdx.x * 64;
  const int64_t s = s_wave + lane;
  if (s >= a.n_samples) return;
  const bool full = a.n_samples - s_wave >= 64;  // wave-uniform
  const bool stg_end = (a.staged & 1) && full, stg_traj = (a.staged & 2) && full;
  const double dt = a.dt;
  const int T = a.n_steps;

  double q[NJ], dq[NJ], tau[NJ];
  {
    const double* __restrict__ qp = a.q + s * a.in_ss;  // (the end state may alias the initial state: read whole before the first store)
    const double* __restrict__ dqp = a.dq + s * a.in_ss;
#pragma unroll
    for (int f = 0; f < NJ; ++f)
    {
      const int idx = c->j[f].in_idx;
      q[f] = idx >= 0 ? qp[idx * a.in_sj] : 0.0;
      dq[f] = idx >= 0 ? dqp[idx * a.in_sj] : 0.0;
      tau[f] = 0.0;
    }
  }
  const double* tp = a.tau + s * a.in_ss;
  if (T > 0)
  {
#pragma unroll
    for (int f = 0; f < NJ; ++f)
    {
      const int idx = c->j[f].in_idx;
      if (idx >= 0) tau[f] = tp[idx * a.in_sj];
    }
  }
  SmallRecords sm;
  if (stg_end || stg_traj)
  {
    extern __shared__ __attribute__((aligned(16))) char rollout_stage_lds[];
    sm.init(rollout_stage_lds, c->n_active, lane);
  }
  const double qnan = __builtin_nan("");
  bool alive = true;
  int due = a.traj_every;  // steps until the next trajectory record
  int64_t rec_off = 0;     // ... and where it goes

#pragma unroll 1
  for (int t = 0; t < T; ++t)
  {
    const bool more = t + 1 < T;
    tp += a.tau_step;
    bool ok = true;
    RDYN_ROLLOUT_HEAD
    if (INTEGRATOR == RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER)
    {
      double rhs[NJ];
#pragma unroll
      for (int f = 0; f < NJ; ++f) rhs[f] = tau[f];
      RDYN_ROLLOUT_TAKE
      if (more)
      {
#pragma unroll
        for (int f = 0; f < NJ; ++f)
        {
          const int idx = c->j[f].in_idx;
          if (idx >= 0) tau[f] = tp[idx * a.in_sj];
        }
        RDYN_ROLLOUT_PREFETCH
      }
      RDYN_ROLLOUT_RHS(q, dq, rhs)
      ok = RDYN_ROLLOUT_EVAL(per_evaluation(c), q, dq, rhs);
#pragma unroll
      for (int f = 0; f < NJ; ++f)
      {
        dq[f] = fma(dt, rhs[f], dq[f]);
        q[f] = fma(dt, dq[f], q[f]);
      }
    }
    else
    {
      double aq[NJ], av[NJ], kq[NJ], kv[NJ];  // weighted sums of the slopes; the last stage's slopes (kv is dead during an evaluation)
#pragma unroll
      for (int f = 0; f < NJ; ++f) aq[f] = av[f] = kq[f] = kv[f] = 0.0;
#pragma unroll 1
      for (int stage = 0; stage < 4; ++stage)
      {
        const double cdt = stage == 0 ? 0.0 : (stage == 3 ? dt : 0.5 * dt);
        const double wgt = (stage == 0 || stage == 3) ? 1.0 / 6.0 : 1.0 / 3.0;
        double sq[NJ], rhs[NJ];
#pragma unroll
        for (int f = 0; f < NJ; ++f)
        {
          sq[f] = fma(cdt, kq[f], q[f]);   // stage 0: q, dq themselves (the slopes start at 0)
          kq[f] = fma(cdt, kv[f], dq[f]);  // the stage velocity = this stage's slope of q
          rhs[f] = tau[f];
        }
        RDYN_ROLLOUT_TAKE
        if (stage == 3 && more)
        {
#pragma unroll
          for (int f = 0; f < NJ; ++f)
          {
            const int idx = c->j[f].in_idx;
            if (idx >= 0) tau[f] = tp[idx * a.in_sj];
          }
          RDYN_ROLLOUT_PREFETCH
        }
        RDYN_ROLLOUT_RHS(sq, kq, rhs)
        ok = RDYN_ROLLOUT_EVAL(per_evaluation(c), sq, kq, rhs) && ok;
#pragma unroll
        for (int f = 0; f < NJ; ++f)
        {
          kv[f] = rhs[f];
          aq[f] = fma(wgt, kq[f], aq[f]);
          av[f] = fma(wgt, kv[f], av[f]);
        }
      }
#pragma unroll
      for (int f = 0; f < NJ; ++f)
      {
        q[f] = fma(dt, aq[f], q[f]);
        dq[f] = fma(dt, av[f], dq[f]);
      }
    }
    alive = alive && ok;
#pragma unroll
    for (int f = 0; f < NJ; ++f)
    {
      q[f] = alive ? q[f] : qnan;
      dq[f] = alive ? dq[f] : qnan;
    }
    if (a.traj_every > 0 && --due == 0)
    {
      due = a.traj_every;
      if (a.q_traj) put_record<NJ>(c, sm, stg_traj, q, a.q_traj + rec_off + s_wave * a.in_ss, a.q_traj + rec_off + s * a.in_ss, a.in_sj, lane);
      if (a.dq_traj) put_record<NJ>(c, sm, stg_traj, dq, a.dq_traj + rec_off + s_wave * a.in_ss, a.dq_traj + rec_off + s * a.in_ss, a.in_sj, lane);
      rec_off += a.traj_step;
    }
  }

  if (a.status) a.status[s] = alive ? 1 : -1;
  if (a.q_end) put_record<NJ>(c, sm, stg_end, q, a.q_end + s_wave * a.in_ss, a.q_end + s * a.in_ss, a.in_sj, lane);
  if (a.dq_end) put_record<NJ>(c, sm, stg_end, dq, a.dq_end + s_wave * a.in_ss, a.dq_end + s * a.in_ss, a.in_sj, lane);
#ifdef RDYN_ROLLOUT_HEAD_DEFAULTED
#undef RDYN_ROLLOUT_HEAD
#undef RDYN_ROLLOUT_HEAD_DEFAULTED
#endif
