"""Test support for the parameter gradients of the closed-loop rollouts (rdyn_rollout_adjoint_feedback_parameters /
Chain.rolloutParameterAdjoint(feedback=) / autograd.closed_loop_rollout): the numpy recomposition over the library's own products with
their parameter rows, a wrapper of the library call (host arrays in, host arrays out), and the oracle-side measurements behind the
central-difference tests with their recorded figures.  torch is an argument, never imported at module level."""
import numpy as np

from _arrays import DT, _dev, _dev_seq, _direction, _host, _host_seq
from _chains import GRAV, _spec
from _feedback import Law, _np_closed_loop
from _feedback_adjoint import (DIRECTIONAL_MODES, DIRECTIONAL_T, LAW_OUTPUTS, _directional_case, _lib_closures, _loss_terms, _np_fb_adjoint,
                               _same_pattern)
from _references import _oracle_fd

CD_CHAINS = ["planar_2r", "ur10_like", "panda_like"]
CD_H = 1.0                       # times _direction(pi): the parameters move by at most 1 % and 0.5 %
LIMIT_STEPS = (1e-1, 1e-2, 1e-3)   # times _direction(pi), the candidates of the test with limits
LIMIT_MODES = [("semi_implicit_euler", True), ("rk4", True)]


class Rows(object):
    """the library's product for _np_fb_adjoint that also adds up the parameter rows of every product it is asked for: the rows are taken
    at the command u the product is taken at, and at its seed"""

    def __init__(self, torch, chain, components):
        self.torch, self.chain, self.cs = torch, chain, components
        self.pi = self.comp = self.api = self.acomp = 0.0

    def __call__(self, q, v, u, seed):
        t = [_dev(self.torch, x, "sample") for x in (q, v, u, seed)]
        out = self.chain.getJointAccelerationVjp(*t, components=self.cs)
        assert (out[0].cpu().numpy() == 1).all()
        rows = self.chain.getJointAccelerationParameterVjp(*t, components=self.cs)
        pi = rows[0].cpu().numpy()
        self.pi, self.api = self.pi + pi, self.api + np.abs(pi)
        if rows[1] is not None:
            comp = rows[1].cpu().numpy()
            self.comp, self.acomp = self.comp + comp, self.acomp + np.abs(comp)
        return tuple(x.cpu().numpy() for x in out[1:])


def _expected(torch, chain, cs, law, q0, dq0, qt, vt, T, gq, gv, rq, rv, gu, integrator, hold, keep=None):
    """(gpi, |gpi| terms, gcomp, |gcomp| terms) by the numpy recomposition of the closed-loop adjoint; keep: the samples that count"""
    rows = Rows(torch, chain, cs)
    fd = _lib_closures(torch, chain, chain, cs)[0]
    _np_fb_adjoint(rows, fd, law, q0, dq0, qt, vt, T, gq, gv, DT, integrator, hold, gq_traj=rq, gdq_traj=rv, gu=gu)
    keep = slice(None) if keep is None else keep
    if cs is None:
        return rows.pi[keep].sum(axis=0), rows.api[keep].sum(axis=0), None, None
    return rows.pi[keep].sum(axis=0), rows.api[keep].sum(axis=0), rows.comp[keep].sum(axis=0), rows.acomp[keep].sum(axis=0)


def _within(got, want, terms, factor, what):
    err = np.abs(got - want)
    worst = float((err / np.where(terms > 0, terms, 1.0)).max())
    assert (err <= factor * terms).all(), (what, worst)
    return worst


def _fbp_adjoint(torch, chain, fw, integrator, layout="sample", gq_end=None, gdq_end=None, gq_traj=None, gdq_traj=None, gu=None,
                 want=LAW_OUTPUTS, dt=DT, **kw):
    """Chain.rolloutParameterAdjoint(feedback=) on _feedback_adjoint._fb_forward's tensors: a dict of host arrays with _fb_adjoint's keys
    and gpi, gcomp (None without components)"""
    d = lambda x: None if x is None else (_dev_seq(torch, x, layout) if x.ndim == 3 else _dev(torch, x, layout))
    tq, tdq, ttau, q_traj, dq_traj, fb = fw[:6]
    want = tuple(k for k in want if not (k in ("Dq_ref", "kd") and fb.kd is None) and not (k == "tau_limit" and fb.tau_limit is None))
    r = chain.rolloutParameterAdjoint(tq, tdq, ttau, dt, q_traj, dq_traj, gq_end=d(gq_end), gDq_end=d(gdq_end), gq_traj=d(gq_traj),
                                      gDq_traj=d(gdq_traj), integrator=integrator, layout=layout, feedback=fb, want_feedback=want,
                                      gu_traj=d(gu), **kw)
    host = lambda t: _host_seq(t, layout) if t.dim() == 3 else _host(t, layout)
    res = {"gq0": _host(r[0], layout), "gdq0": _host(r[1], layout), "gtau": host(r[2]), "gpi": r[3].cpu().numpy(),
           "gcomp": None if r[4] is None else r[4].cpu().numpy(), "status": r[5].cpu().numpy()}
    names = {"q_ref": "gq_ref", "Dq_ref": "gdq_ref", "kp": "gkp", "kd": "gkd", "tau_limit": "glim"}
    for k, t in zip(want, r[6:]):
        res[names[k]] = host(t)
    return res


def _clamped_share(u, lim):
    """the share of the entries of a command record (T, N, n) that sit at a limit"""
    return float((np.abs(u) == lim).mean())


# ---- central differences over the model (tests 6 and 7 of test_gpu_rollout_feedback_parameter_adjoint.py)
# The setting of _feedback_adjoint._directional_case (N = 200, T = 8, dt = 1e-3, the gains GAIN_FACTOR was found for, no wrenches) and its
# loss _loss_terms (end state, trajectory records, command record); delta = _direction(pi).  Per sample
#     err(h) = |(L(pi + h delta) - L(pi - h delta)) / (2 h) - <gpi, delta>| / scale,
# scale = the largest |<gpi_link, delta_link>| over the links, as tests/test_parameter_gradient_inputs.py defines them.  On the oracle the
# chain is rebuilt from the perturbed parameters, the closed loop runs through _np_closed_loop, and <gpi, delta> is the Richardson
# extrapolation (4 CD(h / 2) - CD(h)) / 3: err(h) = 4 / 3 |CD(h) - CD(h / 2)|.
def _oracle_with_parameters(name, pi):
    """the oracle chain of `name` with the child links' parameters pi ([m, m c, I about the link origin] per link)"""
    from oracle import oracle as orc
    xml, base, tool, inputs = _spec(name)
    spec = orc.urdf_model.load(xml, base, tool, GRAV, inputs)
    for l, link in enumerate(spec.links[1:]):
        m, h = pi[10 * l], pi[10 * l + 1:10 * l + 4]
        if m == 0.0:   # a massless link stays one (its direction is zero)
            assert not pi[10 * l:10 * l + 10].any()
            link.has_inertial, link.mass, link.xyz, link.quat, link.inertia = True, 0.0, [0.0, 0.0, 0.0], (0.0, 0.0, 0.0, 1.0), [0.0] * 6
            continue
        c = h / m
        Io = pi[10 * l + 4:10 * l + 10]
        cc = m * np.array([c[1] ** 2 + c[2] ** 2, -c[0] * c[1], -c[0] * c[2], c[0] ** 2 + c[2] ** 2, -c[1] * c[2], c[0] ** 2 + c[1] ** 2])
        link.has_inertial, link.mass, link.xyz, link.quat, link.inertia = True, float(m), [float(x) for x in c], (0.0, 0.0, 0.0, 1.0), [float(x) for x in Io - cc]
    real = orc.urdf_model.load
    orc.urdf_model.load = lambda *a, **k: spec
    try:
        return orc.OracleChain(xml, base, tool, GRAV, input_joint_names=inputs)
    finally:
        orc.urdf_model.load = real


def _pi_of(name):
    from rosdyn_amd import Chain
    xml, base, tool, _ = _spec(name)
    return Chain(xml, base, tool, GRAV).getNominalParameters()


def _case(name, n, limits=False):
    """(inputs, seeds) of _directional_case without its wrenches"""
    x, seeds, _ = _directional_case(name, n, 1, limits)
    x = dict(x, W=None)
    return x, seeds


def _oracle_run(name, pi, x, seeds, integrator, hold):
    """(L, the sum of the absolute terms of L, the command record) of the oracle's closed loop on the model pi"""
    ref = _oracle_with_parameters(name, pi)
    rec = []
    law = Law(x["tau"], x["q_ref"], x["kp"], x["kd"], x["dq_ref"], x.get("lim"))
    qe, ve = _np_closed_loop(_oracle_fd(ref), law, x["q0"], x["dq0"], DIRECTIONAL_T, DT, integrator, hold, rec)
    q_traj = np.array([r[0] for r in rec[1:]] + [qe])
    v_traj = np.array([r[1] for r in rec[1:]] + [ve])
    u = np.array([r[3] for r in rec])
    return _loss_terms(seeds, qe, ve, q_traj, v_traj, u) + (u,)


def _link_directions(delta):
    for l in range(len(delta) // 10):
        d = np.zeros_like(delta)
        d[10 * l:10 * l + 10] = delta[10 * l:10 * l + 10]
        yield d


def measure_smooth(name, integrator, hold):
    """err(H) / scale per sample on the oracle alone, without limits"""
    pi = _pi_of(name)
    delta = _direction(pi)
    n = _oracle_with_parameters(name, pi).n
    x, seeds = _case(name, n)
    loss = lambda p: _oracle_run(name, p, x, seeds, integrator, hold)[0]
    cd = lambda d, h: (loss(pi + h * d) - loss(pi - h * d)) / (2.0 * h)
    big, small = cd(delta, CD_H), cd(delta, 0.5 * CD_H)
    err = np.abs(big - (4.0 * small - big) / 3.0)
    terms = [np.abs(cd(d, 0.5 * CD_H)) for d in _link_directions(delta)]
    return err / np.max(terms, axis=0)


def measure_limits(name):
    """(step, {integrator: kept share at the step}, {integrator: worst |CD(h) - CD(h / 2)| / scale over the samples kept at both steps},
    clamped share of the unperturbed RK4 run) on the oracle alone, under hold = 1.  The step is the largest of LIMIT_STEPS at which at
    least half of the samples keep their clamp pattern under both integrators; scale as above, its per-link terms measured at h / 2 over
    the samples kept."""
    pi = _pi_of(name)
    delta = _direction(pi)
    n = _oracle_with_parameters(name, pi).n
    x, seeds = _case(name, n, limits=True)
    lim = x["lim"]
    runs = {}

    def run(integrator, d_key, d, h):
        key = (integrator, d_key if h else None, h)
        if key not in runs:
            runs[key] = _oracle_run(name, pi + h * d, x, seeds, integrator, True)
        return runs[key]

    def kept(integrator, steps):
        u0 = run(integrator, None, delta, 0.0)[2]
        return _same_pattern(lim, u0, *((run(integrator, "all", delta, s)[2], lim) for h in steps for s in (h, -h)))

    step = None
    for h in LIMIT_STEPS:
        if all(kept(i, (h,)).mean() >= 0.5 for i, _ in LIMIT_MODES):
            step = h
            break
    share, noise = {}, {}
    for integrator, _ in LIMIT_MODES:
        share[integrator] = float(kept(integrator, (step,)).mean())
        k = kept(integrator, (step, 0.5 * step))
        cd = [(run(integrator, "all", delta, s)[0] - run(integrator, "all", delta, -s)[0]) / (2.0 * s) for s in (step, 0.5 * step)]
        terms = [np.abs(run(integrator, l, d, 0.5 * step)[0] - run(integrator, l, d, -0.5 * step)[0]) / step
                 for l, d in enumerate(_link_directions(delta))]
        noise[integrator] = float((np.abs(cd[0] - cd[1]) / np.max(terms, axis=0))[k].max())
    u0 = run("rk4", None, delta, 0.0)[2]
    return step, share, noise, _clamped_share(u0, lim)


# (chain, integrator, hold): the oracle's worst err(H) / scale (measure_smooth; every one of the 200 samples qualifies on every row);
# re-measured within 5 % by test_rollout_feedback_parameter_adjoint_inputs.py
FBP_ORACLE_WORST = {
    ('planar_2r', 'semi_implicit_euler', True): 8.306e-04,
    ('planar_2r', 'rk4', True): 8.172e-04,
    ('planar_2r', 'rk4', False): 4.838e-04,
    ('ur10_like', 'semi_implicit_euler', True): 8.289e-03,
    ('ur10_like', 'rk4', True): 6.477e-03,
    ('ur10_like', 'rk4', False): 1.488e-03,
    ('panda_like', 'semi_implicit_euler', True): 2.716e-03,
    ('panda_like', 'rk4', True): 2.669e-03,
    ('panda_like', 'rk4', False): 4.114e-04,
}

# chain: the step of the test with limits (measure_limits: already at 1e-1 the oracle keeps 99 - 100 % of the samples under both
# integrators; 48 - 52 % of the commands of the unperturbed run are clamped); (chain, integrator): the oracle's own
# |CD(h) - CD(h / 2)| / scale there -- at so large a step three quarters of the truncation of CD(h), not rounding
FBP_LIMIT_STEP = {'planar_2r': 1e-1, 'ur10_like': 1e-1, 'panda_like': 1e-1}
FBP_LIMIT_NOISE = {
    ('planar_2r', 'semi_implicit_euler'): 8.061e-05,
    ('planar_2r', 'rk4'): 1.024e-04,
    ('ur10_like', 'semi_implicit_euler'): 4.919e-05,
    ('ur10_like', 'rk4'): 4.896e-05,
    ('panda_like', 'semi_implicit_euler'): 1.198e-05,
    ('panda_like', 'rk4'): 1.142e-05,
}
MODES = DIRECTIONAL_MODES
