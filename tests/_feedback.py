"""Test support for the closed-loop rollouts (rdyn_rollout_feedback / Chain.rollout(feedback=)): seeded references, gains and limits, the
law and the closed loop in numpy around any forward-dynamics function, the measured bounds of the multi-step tests, and a wrapper of the
library call (host arrays in, host arrays out).  torch is an argument, never imported at module level."""
import numpy as np

from _arrays import DT, EPS, WRENCH_SCALE, _dev, _dev_seq, _dev_w, _host, _host_seq, _inf
from _chains import WRENCH_CHAINS
from _references import _np_step, _oracle_fd, _oracle_fd_ext

T_MULTI, N_MULTI = 8, 200
# the factor on the gains (kp = 100 s, kd = 20 s per joint, s the chain's torque scale) at which the oracle alone keeps the deviation of
# the multi-step measurement below 1e-9 under both integrators and both modes (test_rollout_feedback_inputs.py pins it): the largest of
# 1, 0.3, 0.1.  At the full gains the explicit integrators are unstable at dt = 1e-3 on the light distal links (kd dt / M_jj above 2): the
# oracle's own run diverges within the 8 steps.
GAIN_FACTOR = {"planar_2r": 1.0, "ur10_like": 0.1, "panda_like": 0.1, "mixed_joints": 0.1, "ur10_public": 1.0, "ur10_permuted": 0.1,
               "rev10": 0.3, "ur10_public_long": 0.3, "rev14": 0.3, "gen20_permuted": 0.3}
# the actuator limit of the first joint as a multiple of the chain's torque scale s (_limits grades it along the joints), chosen per chain so that between 20 % and 80 %
# of all (sample, joint, step) commands of the oracle's multi-step run are clamped (test_rollout_feedback_inputs.py asserts the share)
LIMIT_FACTOR = {"planar_2r": 22.0, "ur10_like": 2.4, "panda_like": 2.3, "mixed_joints": 2.3, "ur10_public": 28.0, "ur10_permuted": 2.4,
                "rev10": 9.0, "ur10_public_long": 9.5, "rev14": 9.8, "gen20_permuted": 7.0}


def _scale(name):
    return WRENCH_SCALE[name]


def _gains(name, n):
    """the multi-step tests' shared gains: kp = 100 s, kd = 20 s per joint"""
    s = GAIN_FACTOR[name] * _scale(name)
    return np.full(n, 100.0 * s), np.full(n, 20.0 * s)


def _graded_gains(name, n):
    """shared gains that differ from joint to joint (a law indexed in chain order instead of input order shows): 100 s and 20 s times
    1 .. 1.5 along the input joints"""
    kp, kd = _gains(name, n)
    grade = 1.0 + 0.5 * np.arange(n) / max(n - 1, 1)
    return kp * grade, kd * grade


def _sample_gains(name, n, N, seed):
    """per-sample gains: the graded ones times a factor in 0.5 .. 1.5 of their own per entry"""
    from rosdyn_amd.samples import uniform_pm1
    kp, kd = _graded_gains(name, n)
    return kp * (1.0 + 0.5 * uniform_pm1(seed, (N, n))), kd * (1.0 + 0.5 * uniform_pm1(seed + 1, (N, n)))


def _limits(name, n):
    """(n,) limits, graded 1 .. 1.25 along the input joints"""
    return LIMIT_FACTOR[name] * _scale(name) * (1.0 + 0.25 * np.arange(n) / max(n - 1, 1))


def _refs(q0, dq0, T, seed):
    """(T, N, n) x 2: references within +-0.5 of the initial state"""
    from rosdyn_amd.samples import uniform_pm1
    return q0[None] + 0.5 * uniform_pm1(seed, (T,) + q0.shape), dq0[None] + 0.5 * uniform_pm1(seed + 1, (T,) + q0.shape)


class Law:
    """the law of include/rdyn.h on host arrays.  tau_ff, q_ref, dq_ref: (T, N, n) or (N, n) held over the horizon (dq_ref None: zero); kp,
    kd: (n,) or (N, n) (kd None: no velocity term); lim: (n,) or None"""

    def __init__(self, tau_ff, q_ref, kp, kd=None, dq_ref=None, lim=None):
        self.tau_ff, self.q_ref, self.dq_ref, self.kp, self.kd, self.lim = tau_ff, q_ref, dq_ref, kp, kd, lim

    @staticmethod
    def _at(x, t):
        return x[t] if x.ndim == 3 else x

    def parts(self, t, q, dq):
        """(tau_ff, kp e, kd de) of step t at the state (q, dq)"""
        p = self.kp * (self._at(self.q_ref, t) - q)
        if self.kd is None:
            return self._at(self.tau_ff, t), p, np.zeros_like(p)
        ref = self._at(self.dq_ref, t) if self.dq_ref is not None else 0.0
        return self._at(self.tau_ff, t), p, self.kd * (ref - dq)

    def raw(self, t, q, dq):
        ff, p, d = self.parts(t, q, dq)
        return ff + p + d

    def rounding(self, t, q, dq):
        """4 EPS (|tau_ff| + kp |e| + kd |de|) per entry: two fused multiply-adds and two differences of the command"""
        ff, p, d = self.parts(t, q, dq)
        return 4.0 * EPS * (np.abs(ff) + np.abs(p) + np.abs(d))

    def clamp(self, u):
        if self.lim is None:
            return u
        return np.where(u > self.lim, self.lim, np.where(u < -self.lim, -self.lim, u))

    def __call__(self, t, q, dq):
        return self.clamp(self.raw(t, q, dq))


def _np_closed_loop(fd, law, q, dq, T, dt, integrator, hold, record=None):
    """the closed loop in numpy: fd(q, dq, u) the forward dynamics, the command of step t held over the step (hold) or formed at every
    stage.  record: None, or a list that takes (q, dq, raw command, command) of the first evaluation of every step."""
    for t in range(T):
        if record is not None:
            record.append((q, dq, law.raw(t, q, dq), law(t, q, dq)))
        if hold:
            q, dq = _np_step(fd, q, dq, law(t, q, dq), dt, integrator)
        else:
            q, dq = _np_step(lambda a, b, _, t=t: fd(a, b, law(t, a, b)), q, dq, None, dt, integrator)
    return q, dq


def _multi_inputs(name, n, limits=False, seed=9300):
    """the inputs of the multi-step, saturation, record and status tests: (q0, dq0, Law)"""
    from _arrays import _wrench_rollout_inputs
    q0, dq0, tau = _wrench_rollout_inputs(name, n, N_MULTI, T_MULTI, seed=seed)
    q_ref, dq_ref = _refs(q0, dq0, T_MULTI, seed + 10)
    kp, kd = _gains(name, n)
    return q0, dq0, Law(tau, q_ref, kp, kd, dq_ref, _limits(name, n) if limits else None)


def _measure(ref, name, integrator, hold, limits=False):
    """the measurement behind FB_MULTI_STEP, on the CPU with the oracle alone, by the method of test_gpu_rollout.py's MULTI_STEP: the
    closed loop run plain and run with every ddq evaluation multiplied by (1 + 1e-11 xi), xi uniform in +-1 per entry; dev = the largest
    deviation of the end state between the two relative to max(1, |x|_inf) of the sample's (q, dq).  Returns (dev, the plain run's
    record, the plain run's end state)."""
    q0, dq0, law = _multi_inputs(name, ref.n, limits)
    rec = []
    qa, va = _np_closed_loop(_oracle_fd(ref), law, q0, dq0, T_MULTI, DT, integrator, hold, rec)
    qb, vb = _np_closed_loop(_oracle_fd(ref, np.random.default_rng(99)), law, q0, dq0, T_MULTI, DT, integrator, hold)
    scale = np.maximum(1.0, np.maximum(_inf(qa), _inf(va)))
    return float((np.maximum(_inf(qa - qb), _inf(va - vb)) / scale).max()), rec, (qa, va)


# (chain, integrator, hold): dev of _measure without limits; the bound of the multi-step and saturation tests is 8 dev.  Semi-implicit
# Euler is one computation under both modes: one row.
FB_MULTI_STEP = {
    ("planar_2r", "semi_implicit_euler", True): 1.56e-11,
    ("planar_2r", "rk4", True): 1e-11,
    ("planar_2r", "rk4", False): 6.6e-12,
    ("ur10_like", "semi_implicit_euler", True): 9.06e-11,
    ("ur10_like", "rk4", True): 6e-11,
    ("ur10_like", "rk4", False): 8.68e-12,
    ("panda_like", "semi_implicit_euler", True): 2.41e-11,
    ("panda_like", "rk4", True): 2.42e-11,
    ("panda_like", "rk4", False): 1.06e-11,
    ("mixed_joints", "semi_implicit_euler", True): 3.12e-11,
    ("mixed_joints", "rk4", True): 3.56e-11,
    ("mixed_joints", "rk4", False): 6.39e-12,
    ("ur10_public", "semi_implicit_euler", True): 5.72e-10,
    ("ur10_public", "rk4", True): 5.66e-10,
    ("ur10_public", "rk4", False): 8.18e-10,
    ("ur10_permuted", "semi_implicit_euler", True): 5.31e-11,
    ("ur10_permuted", "rk4", True): 4.42e-11,
    ("ur10_permuted", "rk4", False): 7.12e-12,
    ("rev10", "semi_implicit_euler", True): 1.63e-10,
    ("rev10", "rk4", True): 9.67e-11,
    ("rev10", "rk4", False): 2.71e-11,
    ("ur10_public_long", "semi_implicit_euler", True): 2.09e-10,
    ("ur10_public_long", "rk4", True): 6.21e-11,
    ("ur10_public_long", "rk4", False): 3.6e-10,
    ("rev14", "semi_implicit_euler", True): 8.48e-11,
    ("rev14", "rk4", True): 3.82e-11,
    ("rev14", "rk4", False): 3.45e-11,
    ("gen20_permuted", "semi_implicit_euler", True): 8.19e-11,
    ("gen20_permuted", "rk4", True): 3.05e-11,
    ("gen20_permuted", "rk4", False): 1.43e-11,
}


def _bound(name, integrator, hold):
    return 8.0 * FB_MULTI_STEP[(name, integrator, True if integrator == "semi_implicit_euler" else bool(hold))]


def _fb_rollout(torch, chain, q, dq, law, integrator, layout="sample", hold=True, n_steps=None, command_trajectory=False, W=None, link=None,
                wseq=False, **kw):
    """Chain.rollout(feedback=) on host arrays: the state results as _arrays._rollout returns them, then the command trajectory
    (records, N, n) when asked for.  W: None, or host wrenches of one step ((T, ...) with wseq)"""
    from rosdyn_amd import Feedback
    seq = lambda x: None if x is None else (_dev_seq(torch, x, layout) if x.ndim == 3 else _dev(torch, x, layout))
    gain = lambda g: None if g is None else (torch.from_numpy(np.ascontiguousarray(g)).cuda() if g.ndim == 1 else _dev(torch, g, layout))
    fb = Feedback(seq(law.q_ref), gain(law.kp), gain(law.kd), seq(law.dq_ref), hold=hold, tau_limit=gain(law.lim),
                  command_trajectory=command_trajectory)
    if W is not None:
        kw["ext_wrenches"] = torch.stack([_dev_w(torch, w, layout) for w in W]) if wseq else _dev_w(torch, W, layout)
        kw["ext_link"] = None if link is None else chain.getLinksName()[link]
    r = chain.rollout(_dev(torch, q, layout), _dev(torch, dq, layout), seq(law.tau_ff), DT, integrator=integrator, n_steps=n_steps,
                      layout=layout, feedback=fb, **kw)
    out = (_host(r[0], layout), _host(r[1], layout), r[2].cpu().numpy())
    return out + tuple(_host_seq(t, layout) for t in r[3:])
