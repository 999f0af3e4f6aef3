"""Test support for the adjoint of the closed-loop rollouts (rdyn_rollout_adjoint_feedback / Chain.rolloutAdjoint(feedback=)): the
closed-loop adjoint in numpy, written from the formulas of include/rdyn.h around any product `vjp` and forward dynamics `fd`, the same
composition on magnitudes (the bound of the one-step test), and a wrapper of the library call (host arrays in, host arrays out).  torch is
an argument, never imported at module level."""
import numpy as np

from _arrays import DT, _dev, _dev_seq, _dev_w, _host, _host_seq, _host_w, _mat
from _feedback import Law
from _references import _np_step_adjoint, _tau_e, _wrench_matrix

LAW_OUTPUTS = ("q_ref", "Dq_ref", "kp", "kd", "tau_limit")
NEAR = 1e-9   # a raw command within NEAR * lim of a limit: the sample's branch is not pinned, the limits test leaves the sample out


def _at(x, t):
    return x[t] if x.ndim == 3 else x


class Transpose:
    """the law's transpose at one evaluation, accumulating gkp / gkd / glim over the evaluations it sees.  mag: the same composition on
    magnitudes -- every term in absolute value, the mask unchanged -- the sum of the absolute terms of every entry."""

    def __init__(self, law, shape, mag=False):
        self.law, self.mag = law, mag
        self.gkp, self.gkd, self.glim = np.zeros(shape), np.zeros(shape), np.zeros(shape)
        self.near = np.zeros(shape[0], dtype=bool)

    def __call__(self, t, q, v, tot):
        """tot = tau_bar_total + gu -> (the correction of q_bar, of v_bar, g)"""
        law = self.law
        a = np.abs if self.mag else (lambda x: x)
        raw = law.raw(t, q, v)
        hi = lo = np.zeros(raw.shape, dtype=bool)
        if law.lim is not None:
            hi, lo = raw > law.lim, raw < -law.lim
            self.near |= (np.abs(np.abs(raw) - law.lim) <= NEAR * law.lim).any(axis=1)
        g = np.where(hi | lo, 0.0, tot)
        self.gkp += a(_at(law.q_ref, t) - q) * g
        dcorr = np.zeros_like(g)
        if law.kd is not None:
            ref = _at(law.dq_ref, t) if law.dq_ref is not None else 0.0
            self.gkd += a(ref - v) * g
            dcorr = -law.kd * g
        self.glim += np.where(hi, tot, np.where(lo, tot if self.mag else -tot, 0.0))
        if self.mag:
            return law.kp * g, -dcorr, g
        return -law.kp * g, dcorr, g


def _np_fb_adjoint(vjp, fd, law, q0, dq0, q_traj, dq_traj, T, gq_end, gdq_end, dt, integrator, hold, gq_traj=None, gdq_traj=None, gu=None,
                   mag=False):
    """The closed-loop adjoint over the horizon, by the formulas of include/rdyn.h in their order.  vjp(q, v, u, seed) -> (q_bar, v_bar,
    tau_bar) and fd(q, v, u) at the COMMAND u; law: _feedback.Law; x_t from the trajectory given (record k = x_{k + 1}); gu: None or (T,
    N, n) seeds on the command of each step's first evaluation.  mag: everything on magnitudes (vjp then the product on magnitudes, the
    seeds in absolute value).  Returns a dict of gq0, gdq0, gtau, gq_ref, gdq_ref (T, N, n), gkp, gkd, glim (N, n) and near (N,)."""
    a = np.abs if mag else (lambda x: x)
    tr = Transpose(law, q0.shape, mag)
    lq, lv = a(gq_end).copy(), a(gdq_end).copy()
    if gq_traj is not None and T > 0:
        lq, lv = lq + a(gq_traj[T - 1]), lv + a(gdq_traj[T - 1])
    gtau = np.zeros((T,) + q0.shape)
    held = hold or integrator == "semi_implicit_euler"
    for t in range(T - 1, -1, -1):
        q, v = (q0, dq0) if t == 0 else (q_traj[t - 1], dq_traj[t - 1])
        gu_t = a(gu[t]) if gu is not None else 0.0
        if held:
            lq, lv, tb = _np_step_adjoint(vjp, fd, q, v, law(t, q, v), lq, lv, dt, integrator)
            cq, cv, gtau[t] = tr(t, q, v, tb + gu_t)
            lq, lv = lq + cq, lv + cv
        else:
            calls = [0]

            def vjp_law(qs, vs, _, seed, t=t, gu_t=gu_t, calls=calls):
                qb, vb, tb = vjp(qs, vs, law(t, qs, vs), seed)
                calls[0] += 1
                cq, cv, g = tr(t, qs, vs, tb + (gu_t if calls[0] == 4 else 0.0))   # the products run stage 4 .. 1: the first evaluation is the last
                return qb + cq, vb + cv, g

            lq, lv, gtau[t] = _np_step_adjoint(vjp_law, lambda qs, vs, _, t=t: fd(qs, vs, law(t, qs, vs)), q, v, None, lq, lv, dt, integrator)
        if t >= 1 and gq_traj is not None:
            lq, lv = lq + a(gq_traj[t - 1]), lv + a(gdq_traj[t - 1])
    kd = law.kd if law.kd is not None else 0.0
    return {"gq0": lq, "gdq0": lv, "gtau": gtau, "gq_ref": law.kp * gtau, "gdq_ref": kd * gtau, "gkp": tr.gkp, "gkd": tr.gkd,
            "glim": tr.glim, "near": tr.near}


def _lib_closures(torch, chain, chain0, components=None, W=None, link=None):
    """fd, vjp and the product on magnitudes from the library's own calls at host arrays (W: None, or host wrenches (N, L, 6) / (N, 6) with
    link); box["g"] / box["m"] collect the wrench gradient of every product and its magnitude"""
    L = chain.getLinksNumber()
    kw = {"components": components}
    Wl = None
    if W is not None:
        kw["ext_wrenches"] = _dev_w(torch, W, "sample")
        kw["ext_link"] = None if link is None else chain.getLinksName()[link]
        Wl = W
        if link is not None:
            Wl = np.zeros((len(W), L, 6))
            Wl[:, link] = W
    box = {"g": 0.0, "m": 0.0}

    def fd(q, v, u):
        a, st = chain.getJointAcceleration(*(_dev(torch, x, "sample") for x in (q, v, u)), **kw)
        assert (st.cpu().numpy() == 1).all()
        return a.cpu().numpy()

    def vjp(q, v, u, seed):
        want = ("q", "dq", "tau") + (("ext",) if W is not None else ())
        out = chain.getJointAccelerationVjp(*(_dev(torch, x, "sample") for x in (q, v, u, seed)), want=want, **kw)
        assert (out[0].cpu().numpy() == 1).all()
        if W is not None:
            box["g"] = box["g"] + out[4].cpu().numpy()
        return tuple(t.cpu().numpy() for t in out[1:4])

    def avjp(q, v, u, m):
        tau = u - _tau_e(torch, chain0, q, Wl) if W is not None else u
        out = chain.getJointAccelerationDerivatives(*(_dev(torch, x, "sample") for x in (q, v, tau)), components=components)
        Xq, Xv, Mi = (np.abs(_mat(t, "sample")) for t in out[2:])   # [s, i, k]
        w = np.einsum("sik,si->sk", Mi, m)
        if W is not None:
            A = np.abs(_wrench_matrix(torch, chain0, q, L))
            mag = np.einsum("sie,si->se", A, w).reshape(len(q), L, 6)
            box["m"] = box["m"] + (mag if link is None else mag[:, link])
        return np.einsum("sik,si->sk", Xq, m), np.einsum("sik,si->sk", Xv, m), w

    return fd, vjp, avjp, box


def _feedback_of(torch, law, layout, hold, command_trajectory=False):
    """the rosdyn_amd.Feedback of a host Law on the device"""
    from rosdyn_amd import Feedback
    seq = lambda x: None if x is None else (_dev_seq(torch, x, layout) if x.ndim == 3 else _dev(torch, x, layout))
    gain = lambda g: None if g is None else (torch.from_numpy(np.ascontiguousarray(g)).cuda() if g.ndim == 1 else _dev(torch, g, layout))
    return Feedback(seq(law.q_ref), gain(law.kp), gain(law.kd), seq(law.dq_ref), hold=hold, tau_limit=gain(law.lim),
                    command_trajectory=command_trajectory)


def _fb_forward(torch, chain, q0, dq0, law, integrator, hold, layout="sample", W=None, link=None, wseq=False, components=None, dt=DT):
    """the closed-loop forward call with one record per step and the command record: device tensors (tq0, tdq0, ttau_ff, q_traj, dq_traj,
    feedback, tw, link name), the host status and the host command trajectory (T, N, n)"""
    tq, tdq, ttau = _dev(torch, q0, layout), _dev(torch, dq0, layout), _dev_seq(torch, law.tau_ff, layout)
    fb = _feedback_of(torch, law, layout, hold, command_trajectory=True)
    tw = name = None
    if W is not None:
        tw = torch.stack([_dev_w(torch, w, layout) for w in W]) if wseq else _dev_w(torch, W, layout)
        name = None if link is None else chain.getLinksName()[link]
    r = chain.rollout(tq, tdq, ttau, dt, integrator=integrator, layout=layout, trajectory_every=1, components=components, ext_wrenches=tw,
                      ext_link=name, feedback=fb)
    return (tq, tdq, ttau, r[3], r[4], fb, tw, name), r[2].cpu().numpy(), _host_seq(r[5], layout)


def _fb_adjoint(torch, chain, fw, integrator, layout="sample", gq_end=None, gdq_end=None, gq_traj=None, gdq_traj=None, gu=None,
                want=LAW_OUTPUTS, dt=DT, out=None, **kw):
    """Chain.rolloutAdjoint(feedback=) on _fb_forward's tensors: a dict of host arrays gq0, gdq0, gtau, status, gext (with wrenches) and
    gq_ref, gDq_ref, gkp, gkd, gtau_limit as wanted; sequences as (T, N, n), rows as (N, n)"""
    d = lambda x: None if x is None else (_dev_seq(torch, x, layout) if x.ndim == 3 else _dev(torch, x, layout))
    tq, tdq, ttau, q_traj, dq_traj, fb, tw, name = fw
    N = tq.shape[0] if layout == "sample" else tq.shape[1]
    want = tuple(k for k in want if not (k in ("Dq_ref", "kd") and fb.kd is None) and not (k == "tau_limit" and fb.tau_limit is None))
    r = chain.rolloutAdjoint(tq, tdq, ttau, dt, q_traj, dq_traj, gq_end=d(gq_end), gDq_end=d(gdq_end), gq_traj=d(gq_traj), gDq_traj=d(gdq_traj),
                             integrator=integrator, layout=layout, ext_wrenches=tw, ext_link=name, want_ext=tw is not None, feedback=fb,
                             want_feedback=want, gu_traj=d(gu), out=out, **kw)
    host = lambda t: _host_seq(t, layout) if t.dim() == 3 else _host(t, layout)
    res = {"gq0": _host(r[0], layout), "gdq0": _host(r[1], layout), "gtau": host(r[2]), "status": r[3].cpu().numpy()}
    at = 4
    if tw is not None:
        ge = r[4]
        if kw.get("sum_ext"):
            res["gext"] = _host_w(ge, layout, N)
        else:
            res["gext"] = np.array([_host_w(g, layout, N) for g in ge]) if ge.shape[0] else np.zeros((0, N, 6))
        at = 5
    names = {"q_ref": "gq_ref", "Dq_ref": "gdq_ref", "kp": "gkp", "kd": "gkd", "tau_limit": "glim"}
    for k, t in zip(want, r[at:]):
        res[names[k]] = host(t)
    return res


def _law(name, n, N, T, seed, per_sample=False, limits=False, with_kd=True, with_dq_ref=True, q0=None, dq0=None, tau=None):
    """a Law from _feedback.py's gains, limits and references around (q0, dq0) with the feed-forward tau"""
    from _feedback import _graded_gains, _limits, _refs, _sample_gains
    q_ref, dq_ref = _refs(q0, dq0, T, seed + 20)
    kp, kd = _sample_gains(name, n, N, seed + 30) if per_sample else _graded_gains(name, n)
    return Law(tau, q_ref, kp, kd if with_kd else None, dq_ref if (with_kd and with_dq_ref) else None, _limits(name, n) if limits else None)


# ---- directional consistency without limits (test 6 of test_gpu_rollout_feedback_adjoint.py)
# L = <cq, q_T> + <cv, dq_T> + sum_t <rq_t, q_{t+1}> + <rv_t, dq_{t+1}> + <cu_t, u_t>: linear in the end state, the trajectory records and
# the command record (cu scaled so that its terms are O(1) like the others).  Along a direction d in one input, the central difference
# (L(x + h d) - L(x - h d)) / 2 h of the rollout itself against the adjoint's <gradient, d>; err = |difference| / scale per sample, scale =
# the sum of the absolute terms of L.  The central difference carries a truncation error C h^2 whatever computes it; it is MEASURED on the
# CPU with the oracle's closed loop alone (no gradient enters): t(h) = 4 / 3 |FD(h) - FD(h / 2)| = C h^2 (1 + O(h^2)).  FB_DIRECTIONAL holds
# the worst t(h) / scale over the samples; the GPU test allows twice that figure (test_gpu_rollout_adjoint_ext.py's margin) plus the
# rounding of the difference quotient, 64 EPS / h relative to scale (the two rollouts agree with their exact values to a few ulps of the
# terms of L, the margin of 64 covers the T = 8 steps).  A direction whose oracle figure is below that rounding term is bounded by it alone.
DIRECTIONAL_N, DIRECTIONAL_T = 200, 8
FB_DIRECTIONS = ("x0", "tau", "q_ref", "dq_ref", "kp", "kd", "wrench")
DIRECTIONAL_H = {"x0": 2.0 ** -11, "tau": 2.0 ** -7, "q_ref": 2.0 ** -9, "dq_ref": 2.0 ** -9, "kp": 2.0 ** -9, "kd": 2.0 ** -14, "wrench": 2.0 ** -7}
DIRECTIONAL_CHAINS = ["planar_2r", "mixed_joints", "ur10_like", "panda_like", "ur10_public", "rev10"]
# (semi-implicit Euler under hold = 0 is the same computation as under hold = 1 -- one evaluation per step -- and
# test_euler_gives_the_same_bits_under_both_hold_modes pins that every output carries the same bits: one row serves both)
DIRECTIONAL_MODES = [("semi_implicit_euler", True), ("rk4", True), ("rk4", False)]


def _directional_case(name, n, L, limits=False):
    """(inputs, seeds, directions): inputs = dict of q0, dq0, tau, q_ref, dq_ref, kp, kd (per sample), W, lim ((n,) with limits, else
    None); seeds = (cq, cv, rq, rv, cu)"""
    from rosdyn_amd.samples import uniform_pm1
    from _arrays import WRENCH_SCALE, _seeds, _wrench_rollout_inputs, _wrenches
    from _feedback import GAIN_FACTOR
    N, T = DIRECTIONAL_N, DIRECTIONAL_T
    q0, dq0, tau = _wrench_rollout_inputs(name, n, N, T, seed=12900)
    from _feedback import _gains, _refs
    q_ref, dq_ref = _refs(q0, dq0, T, 12905)
    kp, kd = (np.tile(g, (N, 1)) for g in _gains(name, n))   # the gains GAIN_FACTOR was found for, one row per sample so that every sample has its own direction
    law = Law(tau, q_ref, kp, kd, dq_ref)
    x = {"q0": q0, "dq0": dq0, "tau": tau, "q_ref": law.q_ref, "dq_ref": law.dq_ref, "kp": law.kp, "kd": law.kd, "W": _wrenches(name, N, L, seed=12901)}
    cq, cv, rq, rv = _seeds(n, N, T, seed=12910)
    cu = uniform_pm1(12920, (T, N, n)) / (100.0 * WRENCH_SCALE[name] * GAIN_FACTOR[name])
    s = WRENCH_SCALE[name]
    d = {"x0": (uniform_pm1(12930, (N, n)), uniform_pm1(12931, (N, n))), "tau": s * uniform_pm1(12932, (T, N, n)),
         "q_ref": uniform_pm1(12933, (T, N, n)), "dq_ref": uniform_pm1(12934, (T, N, n)), "kp": law.kp * uniform_pm1(12935, (N, n)),
         "kd": law.kd * uniform_pm1(12936, (N, n)), "wrench": _wrenches(name, N, L, seed=12937)}
    x["lim"] = None
    if limits:
        from _feedback import _limits
        x["lim"] = _limits(name, n)
        d["lim"] = x["lim"] * uniform_pm1(12938, (n,))
    return x, (cq, cv, rq, rv, cu), d


def _moved(x, d, what, h):
    y = dict(x)
    if what == "x0":
        y["q0"], y["dq0"] = x["q0"] + h * d["x0"][0], x["dq0"] + h * d["x0"][1]
    else:
        key = "W" if what == "wrench" else what
        y[key] = x[key] + h * d[what]
    return y


def _loss_terms(seeds, q_end, v_end, q_traj, v_traj, u_traj):
    """(L, the sum of the absolute terms of L) per sample"""
    cq, cv, rq, rv, cu = seeds
    terms = np.concatenate([cq * q_end, cv * v_end] + [np.moveaxis(a * b, 0, 1).reshape(len(cq), -1) for a, b in ((rq, q_traj), (rv, v_traj), (cu, u_traj))],
                           axis=1)
    return terms.sum(axis=1), np.abs(terms).sum(axis=1)


def _oracle_loss(ref, x, seeds, integrator, hold):
    from _feedback import _np_closed_loop
    from _references import _oracle_fd_ext
    rec = []
    law = Law(x["tau"], x["q_ref"], x["kp"], x["kd"], x["dq_ref"], x.get("lim"))
    qe, ve = _np_closed_loop(_oracle_fd_ext(ref, x["W"]), law, x["q0"], x["dq0"], DIRECTIONAL_T, DT, integrator, hold, rec)
    q_traj = np.array([r[0] for r in rec[1:]] + [qe])
    v_traj = np.array([r[1] for r in rec[1:]] + [ve])
    u = np.array([r[3] for r in rec])
    return _loss_terms(seeds, qe, ve, q_traj, v_traj, u) + (u,)


def _measure_directional(ref, name, integrator, hold, L):
    """{direction: worst 4 / 3 |FD(h) - FD(h / 2)| / scale} on the oracle alone"""
    x, seeds, d = _directional_case(name, ref.n, L)
    scale = _oracle_loss(ref, x, seeds, integrator, hold)[1]
    out = {}
    for what in FB_DIRECTIONS:
        h = DIRECTIONAL_H[what]
        fd = [(_oracle_loss(ref, _moved(x, d, what, s), seeds, integrator, hold)[0] - _oracle_loss(ref, _moved(x, d, what, -s), seeds, integrator, hold)[0])
              / (2.0 * s) for s in (h, 0.5 * h)]
        out[what] = float((4.0 / 3.0 * np.abs(fd[0] - fd[1]) / scale).max())
    return out


def _directional_bound(name, integrator, hold, what, halved=False):
    """the bound at h = DIRECTIONAL_H[what], or at h / 2 (a quarter of the truncation, twice the rounding)"""
    from _arrays import EPS
    t, h = FB_DIRECTIONAL[(name, integrator, bool(hold))][what], DIRECTIONAL_H[what]
    return (2.0 * t / 4.0 + 64.0 * EPS / (0.5 * h)) if halved else (2.0 * t + 64.0 * EPS / h)


# ---- ... with limits, under hold = 1 (the command record then shows every mask)
# The clamp makes L piecewise smooth: a difference quotient is a derivative only over samples whose clamp pattern -- which entries of the
# command record sit at +lim, at -lim, at neither -- is the same in the unperturbed run and in both perturbed runs; the others are left
# out.  The step is h times the direction (the directions above are of the input's own scale), h the largest of 1e-6, 1e-7, 1e-8 at
# which the ORACLE alone keeps at least half of the samples for every direction and both integrators: FB_LIMIT_STEP.  At such a step
# the quotient is bound by rounding, not truncation: the error of the quotient is MEASURED on the oracle alone as |FD(h) - FD(h / 2)| /
# scale over the samples kept at both steps (rounding of both quotients, and 3 / 4 of what truncation there is): FB_LIMIT_NOISE holds the
# worst figure; the GPU test allows 8 times it (the margin _feedback._bound gives a measured deviation).
LIMIT_STEPS = (1e-6, 1e-7, 1e-8)
LIMIT_DIRECTIONS = FB_DIRECTIONS + ("lim",)
LIMIT_MODES = [("semi_implicit_euler", True), ("rk4", True)]


def _pattern(u, lim):
    """(T, N, n) of +1 / -1 / 0: the command sits at +lim / at -lim / at neither"""
    return np.sign(u) * (np.abs(u) == lim)


def _same_pattern(lim, u0, *others):
    """(N,) bool: every run shows the unperturbed run's pattern; others = (command record, its limits) pairs"""
    p0 = _pattern(u0, lim)
    keep = np.ones(u0.shape[1], dtype=bool)
    for u, l in others:
        keep &= (_pattern(u, l) == p0).all(axis=(0, 2))
    return keep


def _moved_lim(x, d, what, h):
    y = _moved(x, d, what, h) if what != "lim" else dict(x, lim=x["lim"] + h * d["lim"])
    return y


def _measure_limits(ref, name, L):
    """(step, {(integrator, direction): kept share at that step}, {(integrator, direction): noise}, clamped share) on the oracle alone"""
    x, seeds, d = _directional_case(name, ref.n, L, limits=True)
    runs = {}

    def run(integrator, what, h):
        key = (integrator, what if h else None, h)
        if key not in runs:
            runs[key] = _oracle_loss(ref, _moved_lim(x, d, what, h) if h else x, seeds, integrator, True)
        return runs[key]

    def kept(integrator, what, steps):
        u0 = run(integrator, what, 0.0)[2]
        return _same_pattern(x["lim"], u0, *((run(integrator, what, s)[2], _moved_lim(x, d, what, s)["lim"]) for h in steps for s in (h, -h)))

    step = None
    for h in LIMIT_STEPS:
        if all(kept(i, w, (h,)).mean() >= 0.5 for i, _ in LIMIT_MODES for w in LIMIT_DIRECTIONS):
            step = h
            break
    share, noise = {}, {}
    for integrator, _ in LIMIT_MODES:
        scale = run(integrator, None, 0.0)[1]
        for what in LIMIT_DIRECTIONS:
            share[(integrator, what)] = float(kept(integrator, what, (step,)).mean())
            k = kept(integrator, what, (step, 0.5 * step))
            fd = [(run(integrator, what, s)[0] - run(integrator, what, -s)[0]) / (2.0 * s) for s in (step, 0.5 * step)]
            noise[(integrator, what)] = float((np.abs(fd[0] - fd[1]) / scale)[k].max())
    u0 = run("rk4", None, 0.0)[2]
    return step, share, noise, float((_pattern(u0, x["lim"]) != 0).mean())


# (chain, integrator, hold): {direction: the oracle's worst truncation figure}: _measure_directional, re-measured within 5 % by
# test_rollout_feedback_adjoint_inputs.py
FB_DIRECTIONAL = {
    ('planar_2r', 'semi_implicit_euler', True): {'x0': 9.41e-08, 'tau': 4.26e-14, 'q_ref': 3.55e-10, 'dq_ref': 1.21e-12, 'kp': 1.19e-10, 'kd': 4.65e-10, 'wrench': 5.07e-14},
    ('planar_2r', 'rk4', True): {'x0': 9.43e-08, 'tau': 4.82e-14, 'q_ref': 3.41e-10, 'dq_ref': 1.28e-12, 'kp': 9.28e-11, 'kd': 4.67e-10, 'wrench': 6.12e-14},
    ('planar_2r', 'rk4', False): {'x0': 7.52e-08, 'tau': 4.19e-14, 'q_ref': 1.76e-10, 'dq_ref': 8.34e-13, 'kp': 8.58e-11, 'kd': 4.56e-10, 'wrench': 6.18e-14},
    ('mixed_joints', 'semi_implicit_euler', True): {'x0': 2.22e-08, 'tau': 7.72e-14, 'q_ref': 3.52e-12, 'dq_ref': 3.14e-13, 'kp': 1.53e-10, 'kd': 1.72e-09, 'wrench': 1.39e-13},
    ('mixed_joints', 'rk4', True): {'x0': 2.21e-08, 'tau': 8.73e-14, 'q_ref': 3.82e-12, 'dq_ref': 2.24e-13, 'kp': 1.19e-10, 'kd': 1.69e-09, 'wrench': 1.03e-13},
    ('mixed_joints', 'rk4', False): {'x0': 2.28e-08, 'tau': 2.76e-14, 'q_ref': 5.36e-13, 'dq_ref': 9.8e-14, 'kp': 1.17e-10, 'kd': 2.09e-10, 'wrench': 8.49e-14},
    ('ur10_like', 'semi_implicit_euler', True): {'x0': 7.99e-09, 'tau': 1.1e-13, 'q_ref': 9.85e-13, 'dq_ref': 4.03e-13, 'kp': 9.89e-11, 'kd': 9.7e-09, 'wrench': 4.95e-12},
    ('ur10_like', 'rk4', True): {'x0': 8.02e-09, 'tau': 5.78e-14, 'q_ref': 9.86e-13, 'dq_ref': 2.84e-13, 'kp': 7.09e-11, 'kd': 9.6e-09, 'wrench': 5e-12},
    ('ur10_like', 'rk4', False): {'x0': 1.01e-08, 'tau': 2.76e-14, 'q_ref': 4.65e-13, 'dq_ref': 8.03e-14, 'kp': 7.75e-11, 'kd': 2.11e-10, 'wrench': 4.93e-12},
    ('panda_like', 'semi_implicit_euler', True): {'x0': 5.32e-07, 'tau': 8.53e-13, 'q_ref': 1.82e-11, 'dq_ref': 2.32e-13, 'kp': 7.09e-11, 'kd': 9.57e-10, 'wrench': 2.84e-11},
    ('panda_like', 'rk4', True): {'x0': 5.31e-07, 'tau': 1.11e-12, 'q_ref': 1.88e-11, 'dq_ref': 2.13e-13, 'kp': 5.32e-11, 'kd': 9.47e-10, 'wrench': 3.04e-11},
    ('panda_like', 'rk4', False): {'x0': 5.87e-07, 'tau': 1.55e-13, 'q_ref': 1.14e-11, 'dq_ref': 2.23e-13, 'kp': 5.18e-11, 'kd': 1.3e-10, 'wrench': 2.6e-11},
    ('ur10_public', 'semi_implicit_euler', True): {'x0': 3.88e-06, 'tau': 9.29e-11, 'q_ref': 2.73e-06, 'dq_ref': 1.59e-07, 'kp': 4.42e-08, 'kd': 2.82e-07, 'wrench': 9.09e-11},
    ('ur10_public', 'rk4', True): {'x0': 3.66e-06, 'tau': 6.89e-11, 'q_ref': 2.46e-06, 'dq_ref': 1.42e-07, 'kp': 3.39e-08, 'kd': 2.65e-07, 'wrench': 7.33e-11},
    ('ur10_public', 'rk4', False): {'x0': 2.34e-05, 'tau': 9.33e-13, 'q_ref': 9.9e-08, 'dq_ref': 3.71e-10, 'kp': 1.33e-09, 'kd': 4.82e-06, 'wrench': 5.48e-11},
    ('rev10', 'semi_implicit_euler', True): {'x0': 9.29e-07, 'tau': 2.21e-11, 'q_ref': 5.36e-08, 'dq_ref': 4.97e-10, 'kp': 1.35e-09, 'kd': 8.67e-08, 'wrench': 1.38e-12},
    ('rev10', 'rk4', True): {'x0': 9.07e-07, 'tau': 9.24e-12, 'q_ref': 5.07e-08, 'dq_ref': 4.14e-10, 'kp': 6.48e-10, 'kd': 8.95e-08, 'wrench': 1.15e-12},
    ('rev10', 'rk4', False): {'x0': 9.41e-08, 'tau': 8.06e-14, 'q_ref': 6.89e-11, 'dq_ref': 7e-13, 'kp': 7.68e-11, 'kd': 7.73e-09, 'wrench': 1.1e-12},
}

# chain: the step of the directional test with limits (_measure_limits: at 1e-6 the oracle keeps every sample of every chain, and
# 39 - 52 % of the commands of the unperturbed run are clamped); (chain, integrator): the worst noise figure over the directions.
# test_rollout_feedback_adjoint_inputs.py re-measures both
FB_LIMIT_STEP = {'planar_2r': 1e-06, 'mixed_joints': 1e-06, 'ur10_like': 1e-06, 'panda_like': 1e-06, 'ur10_public': 1e-06, 'rev10': 1e-06}
FB_LIMIT_NOISE = {
    ('planar_2r', 'semi_implicit_euler'): 3.45e-10,
    ('planar_2r', 'rk4'): 3.86e-10,
    ('mixed_joints', 'semi_implicit_euler'): 4.18e-10,
    ('mixed_joints', 'rk4'): 3.23e-10,
    ('ur10_like', 'semi_implicit_euler'): 4.26e-10,
    ('ur10_like', 'rk4'): 3.18e-10,
    ('panda_like', 'semi_implicit_euler'): 5.54e-10,
    ('panda_like', 'rk4'): 2.71e-10,
    ('ur10_public', 'semi_implicit_euler'): 7.35e-09,
    ('ur10_public', 'rk4'): 3.59e-09,
    ('rev10', 'semi_implicit_euler'): 2.68e-09,
    ('rev10', 'rk4'): 9.65e-10,
}
