// rdyn_rollout_adjoint_body.inc -- one lane's backward sweep over the horizon of a rollout (the head of rdyn_rollout_adjoint.hip has the
// scheme), included as text by k_rollout_adjoint and k_rollout_adjoint_params so that the first compiles to exactly what it compiled to
// before the second existed.  Expects: template parameters NJ, INTEGRATOR; the kernel argument a (RdynRolloutAdjointArgs).
// RDYN_ADJ_PARAMS 1 (k_rollout_adjoint_params; also expects p, RdynAdjointParamAcc): every product adds its parameter rows -- the ten
// entries per link of link_parameter_row, then the component columns -- to the lane's own accumulators p.acc[col * p.ld + s], zeroed
// here first, and the sample's final verdict goes to p.status[s]: the host sums the columns over the samples that ended alive.
// RDYN_ADJ_EXT 1 (k_rollout_adjoint_ext; RDYN_ADJ_PARAMS 0; the kernel argument is ax, RdynRolloutAdjointExtArgs, a = ax.a): the rollout
// is rdyn_rollout_ext's -- the wrench of step t, held over the step, enters the rebuilt RK4 stages (fwd_dyn_eval_ext) and every product
// (fwd_dyn_vjp_ext_eval) at that stage's own q.  With gw every product ADDS its -(d tau_E / d ext)' w to the lane's own record of the
// step in memory (6 (NJ + 1) doubles per lane do not belong in registers), zeroed when the step begins -- or once, here, when the
// record is the sum over the steps (gw_step = 0): read-modify-write by the one lane that owns it, in the order of the products.
// RDYN_ADJ_FB 1 (k_rollout_adjoint_fb; RDYN_ADJ_PARAMS 0, RDYN_ADJ_EXT either; also expects fb, RdynFeedbackArgs, and gf,
// RdynFeedbackGradArgs): the rollout is rdyn_rollout_feedback's.  The command hook (fb_command, the forward kernel's text) runs before
// each rebuilt stage evaluation and before each product -- at the head of the step over tau[] where the command is held (hold = 1, and
// semi-implicit Euler, written once for both modes), into the evaluation's copy otherwise -- and the law's transpose (fb_transpose)
// after each product (hold = 0 with RK4) or after the step's products (rdyn_rollout_adjoint_fb.hip has the scheme).
#ifndef RDYN_ADJ_FB
#define RDYN_ADJ_FB 0
#define RDYN_ADJ_FB_DEFAULTED
#endif
  const ChainPtr c = as_const(a.chain);
  const int lane = threadIdx.x;
  const int64_t s_wave = (int64_t)blockIdx.x * 64;
  const int64_t s = s_wave + lane;
  if (s >= a.n_samples) return;
  const bool full = a.n_samples - s_wave >= 64;  // wave-uniform
  const bool stg_x = (a.staged & 1) && full, stg_tau = (a.staged & 2) && full;
#if RDYN_ADJ_FB
  const bool stg_ref = gf.staged && full;
#endif
  const double dt = a.dt;
  const int T = a.n_steps;
  const int64_t so = s * a.in_ss;
  SmallRecords sm;
#if RDYN_ADJ_FB
  if (stg_x || stg_tau || stg_ref)
#else
  if (stg_x || stg_tau)
#endif
  {
    extern __shared__ __attribute__((aligned(16))) char adjoint_stage_lds[];
    sm.init(adjoint_stage_lds, c->n_active, lane);
  }
  const double qnan = __builtin_nan("");
#if RDYN_ADJ_PARAMS
  // the lane's accumulators, zeroed; the link hook of a product
  double* const pacc = p.acc + s;
#pragma unroll 1
  for (int k = 0; k < 10 * NJ + p.n_comp_cols; ++k) pacc[k * p.ld] = 0.0;
  auto link = [&](int f, JointRef, V3 om, V3 vl, V3 al, V3 acc, V3 ov, V3 vv) {
    double g[10];
    link_parameter_row(om, vl, al, acc, ov, vv, g);
    double* const x = pacc + (int64_t)(10 * f) * p.ld;
#pragma unroll
    for (int k = 0; k < 10; ++k) x[k * p.ld] += g[k];
  };
#endif

#if RDYN_ADJ_EXT
  const RdynExtArgs& x = ax.x;
  const double* const xp = x.w + s * x.ss;
  ExtEval xe;
  xe.rec = xp;
  xe.se = x.se;
  xe.one = x.one;
  xe.l = xe.a = mk(0, 0, 0);
  const int n_rec = x.one ? 6 : 6 * (NJ + 1);  // doubles of one step's record of the lane
  double* const gwp = ax.gw ? ax.gw + s * x.ss : nullptr;
  double* gw = gwp;  // the record the products of the step add to
  if (gwp && !ax.gw_step)
  {
#pragma unroll 1
    for (int e = 0; e < n_rec; ++e) gwp[e * x.se] = 0.0;
  }
  auto ext_out = [&](int link, V3 lin, V3 ang) {
    if (x.one != 0 && x.one != link + 1) return;  // wave-uniform
    double* const p = gw + (x.one ? 0 : (int64_t)(6 * link) * x.se);
    p[0] += lin.x;
    p[x.se] += lin.y;
    p[2 * x.se] += lin.z;
    p[3 * x.se] += ang.x;
    p[4 * x.se] += ang.y;
    p[5 * x.se] += ang.z;
  };
#endif

  // lambda_T (the end seeds may alias gq0 / gdq0: read whole before the first store)
  double lq[NJ], lv[NJ], gsum[NJ];
  load_record<NJ>(c, a.gq_end ? a.gq_end + so : nullptr, a.in_sj, lq);
  load_record<NJ>(c, a.gdq_end ? a.gdq_end + so : nullptr, a.in_sj, lv);
#pragma unroll
  for (int f = 0; f < NJ; ++f) gsum[f] = 0.0;
  if (T > 0)
  {
    double g[NJ];
    if (a.gq_traj)
    {
      load_record<NJ>(c, a.gq_traj + (int64_t)(T - 1) * a.gtraj_step + so, a.in_sj, g);
#pragma unroll
      for (int f = 0; f < NJ; ++f) lq[f] += g[f];
    }
    if (a.gdq_traj)
    {
      load_record<NJ>(c, a.gdq_traj + (int64_t)(T - 1) * a.gtraj_step + so, a.in_sj, g);
#pragma unroll
      for (int f = 0; f < NJ; ++f) lv[f] += g[f];
    }
  }
  bool alive = true;
#if RDYN_ADJ_FB
  if (!gf.accumulate) fb_rows_fill<NJ>(c, gf, so, a.in_sj, 0.0);
  const bool held = INTEGRATOR == RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER || fb.hold;  // wave-uniform: one command serves the step
#endif

#pragma unroll 1
  for (int t = T - 1; t >= 0; --t)
  {
    double q[NJ], dq[NJ], tau[NJ], gt[NJ];
    {
      const int64_t ro = (int64_t)(t - 1) * a.traj_step + so;
      load_record<NJ>(c, t == 0 ? a.q + so : a.q_traj + ro, a.in_sj, q);
      load_record<NJ>(c, t == 0 ? a.dq + so : a.dq_traj + ro, a.in_sj, dq);
      load_record<NJ>(c, a.tau + (int64_t)t * a.tau_step + so, a.in_sj, tau);
    }
#if RDYN_ADJ_EXT
    xe.rec = xp + (int64_t)t * x.step;
    if (x.one) ext_load6(xe.rec, x.se, xe.l, xe.a);
    if (gwp && ax.gw_step)
    {
      gw = gwp + (int64_t)t * ax.gw_step;
#pragma unroll 1
      for (int e = 0; e < n_rec; ++e) gw[e * x.se] = 0.0;
    }
#endif
    bool ok = true;
#if RDYN_ADJ_FB
    if (held) fb_command<NJ>(c, fb, so, a.in_sj, t, q, dq, tau);  // tau = the command from here on; the transpose loads tau_ff again
#endif
    if (INTEGRATOR == RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER)
    {
      double qb[NJ], vb[NJ];
#pragma unroll
      for (int f = 0; f < NJ; ++f)
      {
        lv[f] = fma(dt, lq[f], lv[f]);
        gt[f] = dt * lv[f];  // mu; the product leaves tau_bar here
      }
#if RDYN_ADJ_PARAMS
      ok = fwd_dyn_vjp_params_eval<NJ>(per_evaluation(c), a.t, [&](int f, int) { return q[f]; }, [&](int f, int) { return dq[f]; }, tau, gt, qb,
                                       vb, true, true, [](bool, double (&)[NJ]) {}, link);
      component_parameter_rows<NJ>(c, a.t, q, dq, gt, pacc + (int64_t)(10 * NJ) * p.ld, p.ld);
#elif RDYN_ADJ_EXT
      ok = fwd_dyn_vjp_ext_eval<NJ>(per_evaluation(c), a.t, [&](int f, int) { return q[f]; }, [&](int f, int) { return dq[f]; }, tau, gt, qb, vb,
                                    true, true, [](bool, double (&)[NJ]) {}, xe, gwp != nullptr, ext_out);
#else
      ok = fwd_dyn_vjp_eval<NJ>(per_evaluation(c), a.t, [&](int f, int) { return q[f]; }, [&](int f, int) { return dq[f]; }, tau, gt, qb, vb, true,
                                true, [](bool, double (&)[NJ]) {});
#endif
#if RDYN_ADJ_FB
      {
        double ff[NJ];
        load_record<NJ>(c, a.tau + (int64_t)t * a.tau_step + so, a.in_sj, ff);
        ok = fb_transpose<NJ>(c, fb, gf, so, a.in_sj, t, true, ff, q, dq, gt, qb, vb) && ok;
      }
#endif
#pragma unroll
      for (int f = 0; f < NJ; ++f)
      {
        lq[f] += qb[f];
        lv[f] += vb[f];
      }
    }
    else
    {
      // ---- the stage states X2 .. X4 (X1 = x_t), rdyn_rollout_body.inc's arithmetic
      double x2q[NJ], x2v[NJ], x3q[NJ], x3v[NJ], x4q[NJ], x4v[NJ];
      {
        double sq[NJ], kq[NJ];
#pragma unroll
        for (int f = 0; f < NJ; ++f)
        {
          sq[f] = q[f];
          kq[f] = dq[f];
          x2q[f] = x2v[f] = x3q[f] = x3v[f] = x4q[f] = x4v[f] = 0.0;
        }
#pragma unroll 1
        for (int stage = 0; stage < 3; ++stage)
        {
          double rhs[NJ];
#if RDYN_ADJ_FB
#pragma unroll
          for (int f = 0; f < NJ; ++f) rhs[f] = tau[f];
          if (!held) fb_command<NJ>(c, fb, so, a.in_sj, t, sq, kq, rhs);  // the continuous law at the stage state, the components behind the clamp
#pragma unroll
          for (int f = 0; f < NJ; ++f)
          {
            const int idx = c->j[f].in_idx;
            if (idx >= 0) rhs[f] -= joint_component_torque(a.t, idx, sq[f], kq[f]);
          }
#else
#pragma unroll
          for (int f = 0; f < NJ; ++f)
          {
            const int idx = c->j[f].in_idx;
            rhs[f] = tau[f];
            if (idx >= 0) rhs[f] -= joint_component_torque(a.t, idx, sq[f], kq[f]);
          }
#endif
#if RDYN_ADJ_EXT
          fwd_dyn_eval_ext<NJ>(per_evaluation(c), sq, kq, rhs, xe);
#else
          fwd_dyn_eval<NJ>(per_evaluation(c), sq, kq, rhs);  // (its pivot test runs again inside the stage's product)
#endif
          const double cdt = stage == 2 ? dt : 0.5 * dt;  // of the NEXT stage
#pragma unroll
          for (int f = 0; f < NJ; ++f)
          {
            sq[f] = fma(cdt, kq[f], q[f]);
            kq[f] = fma(cdt, rhs[f], dq[f]);
            x2q[f] = stage == 0 ? sq[f] : x2q[f];
            x2v[f] = stage == 0 ? kq[f] : x2v[f];
            x3q[f] = stage == 1 ? sq[f] : x3q[f];
            x3v[f] = stage == 1 ? kq[f] : x3v[f];
            x4q[f] = stage == 2 ? sq[f] : x4q[f];
            x4v[f] = stage == 2 ? kq[f] : x4v[f];
          }
        }
      }
      // ---- the four products, last stage first
      double xq[NJ], xv[NJ], cq[NJ], cv[NJ];  // x_bar; the carry c_{i + 1} X_bar_{i + 1} into stage i's seed
#pragma unroll
      for (int f = 0; f < NJ; ++f)
      {
        xq[f] = lq[f];
        xv[f] = lv[f];
        cq[f] = cv[f] = gt[f] = 0.0;
      }
#pragma unroll 1
      for (int i = 3; i >= 0; --i)
      {
        const double dtb = dt * ((i == 0 || i == 3) ? 1.0 / 6.0 : 1.0 / 3.0);
        const double ci = i == 3 ? dt : 0.5 * dt;
        double sq[NJ], sv[NJ], rhs[NJ], mu[NJ], qb[NJ], vb[NJ];
#pragma unroll
        for (int f = 0; f < NJ; ++f)
        {
          sq[f] = i == 0 ? q[f] : (i == 1 ? x2q[f] : (i == 2 ? x3q[f] : x4q[f]));
          sv[f] = i == 0 ? dq[f] : (i == 1 ? x2v[f] : (i == 2 ? x3v[f] : x4v[f]));
          rhs[f] = tau[f];
          cq[f] = fma(dtb, lq[f], cq[f]);  // kq_i
          mu[f] = fma(dtb, lv[f], cv[f]);  // kv_i
        }
#if RDYN_ADJ_FB
        if (!held) fb_command<NJ>(c, fb, so, a.in_sj, t, sq, sv, rhs);
#endif
#if RDYN_ADJ_PARAMS
        ok = fwd_dyn_vjp_params_eval<NJ>(per_evaluation(c), a.t, [&](int f, int) { return sq[f]; }, [&](int f, int) { return sv[f]; }, rhs, mu,
                                         qb, vb, true, true, [](bool, double (&)[NJ]) {}, link) &&
             ok;
        component_parameter_rows<NJ>(c, a.t, sq, sv, mu, pacc + (int64_t)(10 * NJ) * p.ld, p.ld);
#elif RDYN_ADJ_EXT
        ok = fwd_dyn_vjp_ext_eval<NJ>(per_evaluation(c), a.t, [&](int f, int) { return sq[f]; }, [&](int f, int) { return sv[f]; }, rhs, mu, qb,
                                      vb, true, true, [](bool, double (&)[NJ]) {}, xe, gwp != nullptr, ext_out) &&
             ok;
#else
        ok = fwd_dyn_vjp_eval<NJ>(per_evaluation(c), a.t, [&](int f, int) { return sq[f]; }, [&](int f, int) { return sv[f]; }, rhs, mu, qb, vb,
                                true, true, [](bool, double (&)[NJ]) {}) &&
             ok;
#endif
#if RDYN_ADJ_FB
        if (!held) ok = fb_transpose<NJ>(c, fb, gf, so, a.in_sj, t, i == 0, tau, sq, sv, mu, qb, vb) && ok;  // (tau is tau_ff here)
#endif
#pragma unroll
        for (int f = 0; f < NJ; ++f)
        {
          const double bv = cq[f] + vb[f];  // X_bar_i = (qb, bv)
          gt[f] += mu[f];
          xq[f] += qb[f];
          xv[f] += bv;
          cq[f] = ci * qb[f];
          cv[f] = ci * bv;
        }
      }
#pragma unroll
      for (int f = 0; f < NJ; ++f)
      {
        lq[f] = xq[f];
        lv[f] = xv[f];
      }
#if RDYN_ADJ_FB
      if (held)  // the held command: one transpose at x_t, of the sum of the four stage products, applied to lambda_t
      {
        double ff[NJ];
        load_record<NJ>(c, a.tau + (int64_t)t * a.tau_step + so, a.in_sj, ff);
        ok = fb_transpose<NJ>(c, fb, gf, so, a.in_sj, t, true, ff, q, dq, gt, lq, lv) && ok;
      }
#endif
    }
    alive = alive && ok;
#pragma unroll
    for (int f = 0; f < NJ; ++f)
    {
      lq[f] = alive ? lq[f] : qnan;
      lv[f] = alive ? lv[f] : qnan;
      gt[f] = alive ? gt[f] : qnan;
      gsum[f] += gt[f];
    }
#if RDYN_ADJ_EXT
    if (gwp && ax.gw_step && !alive)
    {
#pragma unroll 1
      for (int e = 0; e < n_rec; ++e) gw[e * x.se] = qnan;
    }
#endif
    if (a.gtau && a.gtau_step)
    {
      const int64_t go = (int64_t)t * a.gtau_step;
      put_record<NJ>(c, sm, stg_tau, gt, a.gtau + go + s_wave * a.in_ss, a.gtau + go + so, a.in_sj, lane);
    }
#if RDYN_ADJ_FB
    fb_reference_gradients<NJ>(c, fb, gf, sm, stg_ref, so, s_wave * a.in_ss, a.in_sj, t, gt, lane);
#endif
    if (t >= 1)
    {
      double g[NJ];
      if (a.gq_traj)
      {
        load_record<NJ>(c, a.gq_traj + (int64_t)(t - 1) * a.gtraj_step + so, a.in_sj, g);
#pragma unroll
        for (int f = 0; f < NJ; ++f) lq[f] += g[f];
      }
      if (a.gdq_traj)
      {
        load_record<NJ>(c, a.gdq_traj + (int64_t)(t - 1) * a.gtraj_step + so, a.in_sj, g);
#pragma unroll
        for (int f = 0; f < NJ; ++f) lv[f] += g[f];
      }
    }
  }

  if (a.status) a.status[s] = alive ? 1 : -1;
#if RDYN_ADJ_EXT
  if (gwp && !ax.gw_step && !alive)
  {
#pragma unroll 1
    for (int e = 0; e < n_rec; ++e) gwp[e * x.se] = qnan;
  }
#endif
#if RDYN_ADJ_PARAMS
  p.status[s] = alive ? 1 : -1;
#endif
#if RDYN_ADJ_FB
  if (!alive) fb_rows_fill<NJ>(c, gf, so, a.in_sj, qnan);
#endif
  if (a.gtau && !a.gtau_step) put_record<NJ>(c, sm, stg_tau, gsum, a.gtau + s_wave * a.in_ss, a.gtau + so, a.in_sj, lane);
  if (a.gq0) put_record<NJ>(c, sm, stg_x, lq, a.gq0 + s_wave * a.in_ss, a.gq0 + so, a.in_sj, lane);
  if (a.gdq0) put_record<NJ>(c, sm, stg_x, lv, a.gdq0 + s_wave * a.in_ss, a.gdq0 + so, a.in_sj, lane);
#ifdef RDYN_ADJ_FB_DEFAULTED
#undef RDYN_ADJ_FB_DEFAULTED
#undef RDYN_ADJ_FB
#endif
