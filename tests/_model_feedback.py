"""Test support for the model-based laws of the closed-loop rollouts (rdyn_rollout_model_feedback / Chain.rollout(feedback=ModelFeedback)):
the wrong model every test runs with, the laws in numpy around the oracle's regressor, the inputs, the measured bounds of the multi-step,
closed-form and saturation tests, and a wrapper of the library call (host arrays in, host arrays out).  torch is an argument, never
imported at module level.
The oracle cannot take other inertial parameters, but the torque is linear in them: the model torque of the references is
regressor(q, v, a) @ pi_hat."""
import numpy as np

from _arrays import DT, EPS, _dev, _dev_seq, _dev_w, _host, _host_seq, _inf
from _feedback import N_MULTI, T_MULTI, Law, _gains, _np_closed_loop, _refs, _scale
from _references import _oracle_fd

CHAINS = ["planar_2r", "ur10_like", "panda_like", "mixed_joints", "ur10_permuted", "ur10_public", "rev10"]
SMALL_CHAINS = ["planar_2r", "ur10_like", "panda_like", "mixed_joints", "ur10_permuted"]   # what the CPU test recomputes
LAWS = ("computed_torque", "gravity_compensation")
CT, GC = LAWS
DDQ_REF_SCALE = 5.0   # rad / s^2: the acceleration reference of the computed-torque law, uniform in +- this


def _pi_hat(pi0):
    """the controller's parameters: test_parameter_gradient_facade.py's perturbation, every entry off by up to 6.25 %"""
    return pi0 * (1.0 + ((np.arange(pi0.size) * 5) % 9 - 4) / 64.0)


def _model(chain):
    return chain.withParameters(_pi_hat(chain.getNominalParameters()))


def _model_torque(ref, pi, perturb=None):
    """RNEA of the model with parameters pi on host arrays, from the oracle's regressor; perturb: a Generator, every torque times
    (1 + 1e-11 xi)"""
    def mt(q, v, a):
        tau = np.einsum("snp,p->sn", ref.regressor(q, v, a), pi)
        if perturb is not None:
            tau = tau * (1.0 + 1e-11 * perturb.uniform(-1.0, 1.0, tau.shape))
        return tau
    return mt


class ModelLaw(Law):
    """the laws of include/rdyn.h (rdyn_rollout_model_feedback) on host arrays: Law's fields, the model torque mt(q, v, a), the law's name
    and (computed torque) ddq_ref, (T, N, n), (N, n) or None"""

    def __init__(self, mt, law, tau_ff, q_ref, kp, kd=None, dq_ref=None, ddq_ref=None, lim=None):
        Law.__init__(self, tau_ff, q_ref, kp, kd, dq_ref, lim)
        assert law in LAWS and (ddq_ref is None or law == CT)
        self.mt, self.law, self.ddq_ref = mt, law, ddq_ref

    def _pd(self, t, q, dq):
        _, p, d = self.parts(t, q, dq)
        return p + d

    def terms(self, t, q, dq):
        """(what the model torque is added to, the model torque)"""
        ff = self._at(self.tau_ff, t)
        if self.law == CT:
            a = self._pd(t, q, dq) + (self._at(self.ddq_ref, t) if self.ddq_ref is not None else 0.0)
            return ff, self.mt(q, dq, a)
        z = np.zeros_like(q)
        return ff + self._pd(t, q, dq), self.mt(q, z, z)

    def raw(self, t, q, dq):
        base, tau_m = self.terms(t, q, dq)
        return base + tau_m

    def rounding(self, t, q, dq):
        """per sample, (N, 1): the model torque within the project's parity bound, 1e-11 max(1, |tau_m|_inf), and the sum's own rounding"""
        base, tau_m = self.terms(t, q, dq)
        return (1e-11 * np.maximum(1.0, _inf(tau_m)) + 4.0 * EPS * (_inf(base) + _inf(tau_m)))[:, None]


def _ct_gains(n):
    """computed torque: kp = 100 / s^2, kd = 20 / s, graded 1 .. 1.5 along the input joints as _feedback._graded_gains grades"""
    grade = 1.0 + 0.5 * np.arange(n) / max(n - 1, 1)
    return 100.0 * grade, 20.0 * grade


def _law_gains(name, n, law):
    """computed torque: the graded gains above; gravity compensation: _feedback._gains, the torque-scaled gains at the chain's GAIN_FACTOR
    (graded 1 .. 1.5 they leave the range in which the oracle's own explicit loop is stable on ur10_public: its run diverges)"""
    return _ct_gains(n) if law == CT else _gains(name, n)


def _sample_law_gains(name, n, N, law, seed):
    """per-sample gains: the shared ones times a factor in 0.5 .. 1 of their own per entry (never above the shared gains: see _law_gains)"""
    from rosdyn_amd.samples import uniform_pm1
    kp, kd = _law_gains(name, n, law)
    return kp * (0.75 + 0.25 * uniform_pm1(seed, (N, n))), kd * (0.75 + 0.25 * uniform_pm1(seed + 1, (N, n)))


# the actuator limit of the first joint as a multiple of the chain's torque scale (graded 1 .. 1.25 along the joints as _feedback._limits
# grades), per chain and law, chosen on the CPU from the oracle's run so that between 20 % and 80 % of all (sample, joint, step) commands
# are clamped under every integrator and mode (test_rollout_model_feedback_inputs.py asserts the share)
LIMIT_FACTOR_CT = {
    ("planar_2r", CT): 8.3, ("planar_2r", GC): 23.0,
    ("ur10_like", CT): 25.0, ("ur10_like", GC): 4.3,
    ("panda_like", CT): 2.0, ("panda_like", GC): 2.7,
    ("mixed_joints", CT): 230.0, ("mixed_joints", GC): 20.0,
    ("ur10_permuted", CT): 30.0, ("ur10_permuted", GC): 4.4,
    ("ur10_public", CT): 36.0, ("ur10_public", GC): 36.0,
    ("rev10", CT): 1.3, ("rev10", GC): 6.7,
}


def _law_limits(name, n, law):
    return LIMIT_FACTOR_CT[(name, law)] * _scale(name) * (1.0 + 0.25 * np.arange(n) / max(n - 1, 1))


def _mf_inputs(ref, name, law, limits=False, per_sample=False, seed=9300, pi=None, perturb=None):
    """the inputs of the multi-step, saturation, record and status tests: (q0, dq0, ModelLaw) -- _feedback._multi_inputs' states, torques
    and references, the wrong model, the law's gains"""
    from rosdyn_amd.samples import uniform_pm1
    from _arrays import _wrench_rollout_inputs
    n = ref.n
    q0, dq0, tau = _wrench_rollout_inputs(name, n, N_MULTI, T_MULTI, seed=seed)
    q_ref, dq_ref = _refs(q0, dq0, T_MULTI, seed + 10)
    ddq_ref = DDQ_REF_SCALE * uniform_pm1(seed + 20, (T_MULTI,) + q0.shape) if law == CT else None
    kp, kd = _sample_law_gains(name, n, N_MULTI, law, seed + 30) if per_sample else _law_gains(name, n, law)
    pi = _pi_hat(ref.nominal_parameters()) if pi is None else pi
    return q0, dq0, ModelLaw(_model_torque(ref, pi, perturb), law, tau, q_ref, kp, kd, dq_ref, ddq_ref, _law_limits(name, n, law) if limits else None)


def _with_torque(law, mt):
    return ModelLaw(mt, law.law, law.tau_ff, law.q_ref, law.kp, law.kd, law.dq_ref, law.ddq_ref, law.lim)


def _measure_model(ref, name, integrator, hold, law, limits=False, per_sample=False):
    """_feedback._measure for a model-based law: the oracle's closed loop run plain and run with every ddq evaluation AND every model
    torque multiplied by (1 + 1e-11 xi); dev = the largest deviation of the end state relative to max(1, |x|_inf) of the sample's (q, dq).
    Returns (dev, the plain run's record, its end state, the plain run's law)."""
    q0, dq0, plain = _mf_inputs(ref, name, law, limits, per_sample)
    rec = []
    qa, va = _np_closed_loop(_oracle_fd(ref), plain, q0, dq0, T_MULTI, DT, integrator, hold, rec)
    rng = np.random.default_rng(99)
    noisy = _with_torque(plain, _model_torque(ref, _pi_hat(ref.nominal_parameters()), rng))
    qb, vb = _np_closed_loop(_oracle_fd(ref, rng), noisy, q0, dq0, T_MULTI, DT, integrator, hold)
    scale = np.maximum(1.0, np.maximum(_inf(qa), _inf(va)))
    return float((np.maximum(_inf(qa - qb), _inf(va - vb)) / scale).max()), rec, (qa, va), plain


# (chain, integrator, hold, law): dev of _measure_model without limits, shared gains; the bound of the multi-step, saturation, component and
# wrench tests is 8 dev.  Semi-implicit Euler is one computation under both modes: one row.
MF_MULTI_STEP = {
    ("planar_2r", "semi_implicit_euler", True, "computed_torque"): 1.56e-11,
    ("planar_2r", "semi_implicit_euler", True, "gravity_compensation"): 1.63e-11,
    ("planar_2r", "rk4", True, "computed_torque"): 1.16e-11,
    ("planar_2r", "rk4", True, "gravity_compensation"): 9.44e-12,
    ("planar_2r", "rk4", False, "computed_torque"): 6.76e-12,
    ("planar_2r", "rk4", False, "gravity_compensation"): 8.8e-12,
    ("ur10_like", "semi_implicit_euler", True, "computed_torque"): 3.19e-11,
    ("ur10_like", "semi_implicit_euler", True, "gravity_compensation"): 8.13e-11,
    ("ur10_like", "rk4", True, "computed_torque"): 3.48e-11,
    ("ur10_like", "rk4", True, "gravity_compensation"): 4.22e-11,
    ("ur10_like", "rk4", False, "computed_torque"): 1.42e-11,
    ("ur10_like", "rk4", False, "gravity_compensation"): 7.89e-12,
    ("panda_like", "semi_implicit_euler", True, "computed_torque"): 3.94e-11,
    ("panda_like", "semi_implicit_euler", True, "gravity_compensation"): 3.25e-11,
    ("panda_like", "rk4", True, "computed_torque"): 5.4e-11,
    ("panda_like", "rk4", True, "gravity_compensation"): 2.27e-11,
    ("panda_like", "rk4", False, "computed_torque"): 2.61e-11,
    ("panda_like", "rk4", False, "gravity_compensation"): 6.19e-12,
    ("mixed_joints", "semi_implicit_euler", True, "computed_torque"): 4.46e-11,
    ("mixed_joints", "semi_implicit_euler", True, "gravity_compensation"): 4.66e-11,
    ("mixed_joints", "rk4", True, "computed_torque"): 5.31e-11,
    ("mixed_joints", "rk4", True, "gravity_compensation"): 3.11e-11,
    ("mixed_joints", "rk4", False, "computed_torque"): 2.58e-11,
    ("mixed_joints", "rk4", False, "gravity_compensation"): 7.05e-12,
    ("ur10_permuted", "semi_implicit_euler", True, "computed_torque"): 3.69e-11,
    ("ur10_permuted", "semi_implicit_euler", True, "gravity_compensation"): 7.52e-11,
    ("ur10_permuted", "rk4", True, "computed_torque"): 2.99e-11,
    ("ur10_permuted", "rk4", True, "gravity_compensation"): 6e-11,
    ("ur10_permuted", "rk4", False, "computed_torque"): 2.02e-11,
    ("ur10_permuted", "rk4", False, "gravity_compensation"): 7e-12,
    ("ur10_public", "semi_implicit_euler", True, "computed_torque"): 4.12e-11,
    ("ur10_public", "semi_implicit_euler", True, "gravity_compensation"): 1.12e-09,
    ("ur10_public", "rk4", True, "computed_torque"): 3.75e-11,
    ("ur10_public", "rk4", True, "gravity_compensation"): 4.62e-10,
    ("ur10_public", "rk4", False, "computed_torque"): 2.4e-11,
    ("ur10_public", "rk4", False, "gravity_compensation"): 7.85e-10,
    ("rev10", "semi_implicit_euler", True, "computed_torque"): 3.08e-11,
    ("rev10", "semi_implicit_euler", True, "gravity_compensation"): 1.66e-10,
    ("rev10", "rk4", True, "computed_torque"): 3.3e-11,
    ("rev10", "rk4", True, "gravity_compensation"): 1.06e-10,
    ("rev10", "rk4", False, "computed_torque"): 1.86e-11,
    ("rev10", "rk4", False, "gravity_compensation"): 5.43e-11,
}


def _mf_bound(name, integrator, hold, law):
    return 8.0 * MF_MULTI_STEP[(name, integrator, True if integrator == "semi_implicit_euler" else bool(hold), law)]


# ---- the closed form: model = plant, computed torque, no limits, tau_ff = 0, a constant set point, ddq_ref = 0
CLOSED_SEED = 9700


def _closed_form_inputs(name, n):
    """(q0, dq0, q_ref (N, n), kp, kd)"""
    from _arrays import _wrench_rollout_inputs
    from rosdyn_amd.samples import uniform_pm1
    q0, dq0, _ = _wrench_rollout_inputs(name, n, N_MULTI, 1, seed=CLOSED_SEED)
    return (q0, dq0, q0 + 0.5 * uniform_pm1(CLOSED_SEED + 10, q0.shape)) + _ct_gains(n)


def _closed_form_end(q0, dq0, q_ref, kp, kd, integrator, T=T_MULTI, dt=DT):
    """the end state of e'' + kd e' + kp e = 0, e = q - q_ref, under the integrator's own linear map, joint by joint: neither the oracle
    nor the library enters.  RK4 (the continuous law, hold = 0): x <- R(h A) x, R(z) = 1 + z + z^2 / 2 + z^3 / 6 + z^4 / 24,
    A = [[0, 1], [-kp, -kd]]; semi-implicit Euler: v <- v + h a(q, v), q <- q + h v."""
    e, v = q0 - q_ref, dq0.copy()
    if integrator == "semi_implicit_euler":
        for _ in range(T):
            v = v + dt * (-kp * e - kd * v)
            e = e + dt * v
        return q_ref + e, v
    for j in range(q0.shape[1]):
        Z = dt * np.array([[0.0, 1.0], [-kp[j], -kd[j]]])
        Z2 = Z @ Z
        R = np.eye(2) + Z + Z2 / 2.0 + Z2 @ Z / 6.0 + Z2 @ Z2 / 24.0
        x = np.stack([e[:, j], v[:, j]])
        for _ in range(T):
            x = R @ x
        e[:, j], v[:, j] = x
    return q_ref + e, v


def _measure_closed_form(ref, name, integrator):
    """the deviation of the oracle's own loop (model = the oracle's chain: fd(q, v, Y pi) - a accumulated over the steps) from the
    recurrence, relative to max(1, |x|_inf) of the sample's end state"""
    q0, dq0, q_ref, kp, kd = _closed_form_inputs(name, ref.n)
    law = ModelLaw(_model_torque(ref, ref.nominal_parameters()), CT, np.zeros_like(q0), q_ref, kp, kd)
    qa, va = _np_closed_loop(_oracle_fd(ref), law, q0, dq0, T_MULTI, DT, integrator, False)
    qc, vc = _closed_form_end(q0, dq0, q_ref, kp, kd, integrator)
    scale = np.maximum(1.0, np.maximum(_inf(qc), _inf(vc)))
    return float((np.maximum(_inf(qa - qc), _inf(va - vc)) / scale).max())


# (chain, integrator): dev of _measure_closed_form; the bound of the closed-form test is 8 dev
MF_CLOSED_FORM = {
    ("planar_2r", "semi_implicit_euler"): 4.44e-16,
    ("planar_2r", "rk4"): 7.22e-16,
    ("ur10_like", "semi_implicit_euler"): 1.94e-15,
    ("ur10_like", "rk4"): 1.31e-15,
    ("panda_like", "semi_implicit_euler"): 3.22e-15,
    ("panda_like", "rk4"): 1.78e-15,
    ("mixed_joints", "semi_implicit_euler"): 4.22e-15,
    ("mixed_joints", "rk4"): 1.94e-15,
    ("ur10_permuted", "semi_implicit_euler"): 2.36e-13,
    ("ur10_permuted", "rk4"): 1.25e-13,
    ("ur10_public", "semi_implicit_euler"): 1.89e-15,
    ("ur10_public", "rk4"): 1.75e-15,
    ("rev10", "semi_implicit_euler"): 2.08e-15,
    ("rev10", "rk4"): 1.46e-15,
}


def _near_a_limit(rec, law):
    """(N,) bool: samples in which a raw command of the oracle's run lies within the law's rounding of a limit, at any step.  rec: the
    record _np_closed_loop filled"""
    near = np.zeros(len(rec[0][0]), dtype=bool)
    for t, (q, dq, raw, _) in enumerate(rec):
        near |= (np.abs(np.abs(raw) - law.lim) <= law.rounding(t, q, dq)).any(axis=1)
    return near


def _mfb_rollout(torch, chain, model, q, dq, law, integrator, layout="sample", hold=True, n_steps=None, command_trajectory=False, W=None, link=None,
                 **kw):
    """Chain.rollout(feedback=ModelFeedback) on host arrays: _feedback._fb_rollout's results.  law: a ModelLaw (its mt is not used: the
    library sweeps `model`)"""
    from rosdyn_amd import ModelFeedback
    seq = lambda x: None if x is None else (_dev_seq(torch, x, layout) if x.ndim == 3 else _dev(torch, x, layout))
    gain = lambda g: None if g is None else (torch.from_numpy(np.ascontiguousarray(g)).cuda() if g.ndim == 1 else _dev(torch, g, layout))
    fb = ModelFeedback(model, law.law, seq(law.q_ref), gain(law.kp), gain(law.kd), seq(law.dq_ref), seq(law.ddq_ref), hold=hold,
                       tau_limit=gain(law.lim), command_trajectory=command_trajectory)
    if W is not None:
        kw["ext_wrenches"] = _dev_w(torch, W, layout)
        kw["ext_link"] = None if link is None else chain.getLinksName()[link]
    r = chain.rollout(_dev(torch, q, layout), _dev(torch, dq, layout), seq(law.tau_ff), DT, integrator=integrator, n_steps=n_steps,
                      layout=layout, feedback=fb, **kw)
    out = (_host(r[0], layout), _host(r[1], layout), r[2].cpu().numpy())
    return out + tuple(_host_seq(t, layout) for t in r[3:])
