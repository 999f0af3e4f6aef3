// rdyn_fwd_dyn_body.inc -- the body of one forward-dynamics evaluation (rdyn_fwd_dyn_body.h), included as text where it runs so that
// k_fwd_dyn compiles to exactly what it was before k_rollout shared it.  Expects: template parameter NJ; ChainPtr c; double rhs[NJ] (in: the
// torque by chain joint, 0 where the joint is not an input joint; out: ddq); RDYN_FWD_Q(f, idx) / RDYN_FWD_DQ(f, idx) = q, dq of chain joint
// f with input index idx >= 0; RDYN_FWD_LINK_WRENCH(f, R, t, fo, no): statements run once the net wrench (fo, no) of link f + 1 is formed,
// R, t the transform of joint f -- nothing in every kernel but those with external wrenches (rdyn_ext_wrench.h), which subtract the link's
// wrench here.  Leaves bool ok (false: a pivot failed, rhs is not to be used).
  // ---- forward: velocities, bias accelerations and the net wrench of every link in its own frame (DDq = 0)
  V3 w = mk(0, 0, 0), vl = mk(0, 0, 0), al = mk(0, 0, 0);
  V3 acc = mk(-c->g[0], -c->g[1], -c->g[2]);  // base "acceleration" -g
  double sv0[NJ], sv1[NJ];
  V3 Fo[NJ], No[NJ];
#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    JointRef J = c->j[f];
    const int type = J.type;
    const int idx = J.in_idx;
    double qf = 0.0, dqf = 0.0;
    if (idx >= 0)
    {
      qf = RDYN_FWD_Q(f, idx);
      dqf = RDYN_FWD_DQ(f, idx);
    }
    if (type == RDYN_REVOLUTE)
    {
      double sn, cs;
      rdyn_sincos(qf, &sn, &cs);
      sv0[f] = sn;
      sv1[f] = 1.0 - cs;
    }
    else
    {
      sv0[f] = qf;
      sv1[f] = 0.0;
    }
    double R[9];
    V3 t;
    joint_transform(J, sv0[f], sv1[f], R, t);
    {
      const V3 wn = rotT(R, w);
      const V3 vn = rotT(R, vl + cross(w, t));
      const V3 aln = rotT(R, al);
      const V3 an = rotT(R, acc + cross(al, t));
      w = wn; vl = vn; al = aln; acc = an;
    }
    const V3 u = ld3(J.u);
    if (type == RDYN_REVOLUTE)
    {
      acc = axpy(acc, cross(vl, u), dqf);
      al = axpy(al, cross(w, u), dqf);
      w = axpy(w, u, dqf);
    }
    else if (type == RDYN_PRISMATIC)
    {
      acc = axpy(acc, cross(w, u), dqf);
      vl = axpy(vl, u, dqf);
    }
    const RDYN_CONST_AS double* pi = J.pi;
    const double m = pi[0];
    const V3 h = ld3(pi + 1);
    const V3 d = acc + cross(w, vl);
    Fo[f] = axpy(cross(al, h) + cross(w, cross(w, h)), d, m);
    No[f] = symv(pi + 4, al) + cross(w, symv(pi + 4, w)) + cross(h, d);
    RDYN_FWD_LINK_WRENCH(f, R, t, Fo[f], No[f])
  }

  // ---- backward: composite bodies, bias torques, the columns of M
  double M[NJ * (NJ + 1) / 2];
  V3 cF[NJ], cN[NJ];  // column f: the momentum of composite body f under joint f's unit twist, in the current frame
  double cm = 0.0, cI[6] = {0, 0, 0, 0, 0, 0};
  V3 ch = mk(0, 0, 0), F = mk(0, 0, 0), N = mk(0, 0, 0);
  double trace = 0.0;
#pragma unroll
  for (int j = NJ - 1; j >= 0; --j)
  {
    JointRef J = c->j[j];
    const int type = J.type;
    const bool act = J.in_idx >= 0;
    const RDYN_CONST_AS double* pi = J.pi;
    cm += pi[0];
    ch = ch + ld3(pi + 1);
#pragma unroll
    for (int i = 0; i < 6; ++i) cI[i] += pi[4 + i];
    F = F + Fo[j];
    N = N + No[j];
    const V3 u = ld3(J.u);
    // momentum under the unit twist (lin, ang): F = m lin + ang x h, N = h x lin + I ang
    if (type == RDYN_REVOLUTE)
    {
      cF[j] = cross(u, ch);
      cN[j] = symv(cI, u);
    }
    else if (type == RDYN_PRISMATIC)
    {
      cF[j] = mk(cm * u.x, cm * u.y, cm * u.z);
      cN[j] = cross(ch, u);
    }
    else
    {
      cF[j] = mk(0, 0, 0);
      cN[j] = mk(0, 0, 0);
    }
    double hj = 0.0;
    if (type == RDYN_REVOLUTE) hj = dot(u, N);
    else if (type == RDYN_PRISMATIC) hj = dot(u, F);
    rhs[j] = act ? rhs[j] - hj : 0.0;
#pragma unroll
    for (int f = j; f < NJ; ++f)
    {
      double v = 0.0;
      if (type == RDYN_REVOLUTE) v = dot(u, cN[f]);
      else if (type == RDYN_PRISMATIC) v = dot(u, cF[f]);
      const bool both = act && c->j[f].in_idx >= 0;
      M[TRI(f, j)] = both ? v : (f == j ? 1.0 : 0.0);
    }
    if (act) trace += M[TRI(j, j)];
    if (j == 0) break;
    // into the parent's frame: x_parent = R x + t
    double R[9];
    V3 t;
    joint_transform(J, sv0[j], sv1[j], R, t);
    {
      const V3 Fp = rot(R, F);
      N = rot(R, N) + cross(t, Fp);
      F = Fp;
    }
#pragma unroll
    for (int f = j; f < NJ; ++f)
    {
      const V3 Fp = rot(R, cF[f]);
      cN[f] = rot(R, cN[f]) + cross(t, Fp);
      cF[f] = Fp;
    }
    ch = composite_to_parent(R, t, cm, ch, cI);
  }

  // ---- M = L L' in place (the diagonal holds 1 / L_jj), L y = rhs, L' x = y
  const double floor = RDYN_FWD_PIVOT_FLOOR * trace;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
  {
    double d = M[TRI(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) d = fma(-M[TRI(j, k)], M[TRI(j, k)], d);
    ok = ok && (c->j[j].in_idx < 0 || d > floor);
    const double inv = 1.0 / sqrt(d);
    M[TRI(j, j)] = inv;
#pragma unroll
    for (int i = j + 1; i < NJ; ++i)
    {
      double v = M[TRI(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) v = fma(-M[TRI(i, k)], M[TRI(j, k)], v);
      M[TRI(i, j)] = v * inv;
    }
  }
#pragma unroll
  for (int i = 0; i < NJ; ++i)
  {
    double v = rhs[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v = fma(-M[TRI(i, k)], rhs[k], v);
    rhs[i] = v * M[TRI(i, i)];
  }
#pragma unroll
  for (int i = NJ - 1; i >= 0; --i)
  {
    double v = rhs[i];
#pragma unroll
    for (int k = i + 1; k < NJ; ++k) v = fma(-M[TRI(k, i)], rhs[k], v);
    rhs[i] = v * M[TRI(i, i)];
  }
