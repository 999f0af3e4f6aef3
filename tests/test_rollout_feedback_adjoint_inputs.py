"""CPU tests (no GPU, the oracle alone): the premises of test_gpu_rollout_feedback_adjoint.py.
- The limits test of its one-step comparison leaves a sample out when a raw command lies within 1e-9 lim of a limit: on the oracle's run of
  the same inputs no evaluation does (asserted: at most 1 % of the samples).
- FB_DIRECTIONAL (tests/_feedback_adjoint.py), the truncation figures behind the directional bounds, re-measured within 5 %.
- The directional test with limits: the step the oracle chooses per chain (FB_LIMIT_STEP), the kept share at that step (at least half, for
  every direction and both integrators), the clamped share of the unperturbed run, and FB_LIMIT_NOISE -- a rounding figure, so it is
  re-measured within a factor of 2, not 5 %."""
import numpy as np
import pytest

from _arrays import DT, _wrench_rollout_inputs as _inputs
from _chains import _trio
from _feedback import _np_closed_loop
from _feedback_adjoint import (DIRECTIONAL_CHAINS, DIRECTIONAL_MODES, FB_DIRECTIONAL, FB_LIMIT_NOISE, FB_LIMIT_STEP, LIMIT_MODES, NEAR, _law,
                               _measure_directional, _measure_limits)
from _references import _oracle_fd

CHAINS = ["planar_2r", "mixed_joints", "ur10_like", "panda_like", "ur10_public", "ur10_permuted", "rev10", "ur10_public_long"]


class _Watch:
    """a Law that records how close every raw command it forms comes to a limit"""

    def __init__(self, law, N):
        self.law, self.near = law, np.zeros(N, dtype=bool)

    def raw(self, t, q, dq):
        return self.law.raw(t, q, dq)

    def __call__(self, t, q, dq):
        raw = self.law.raw(t, q, dq)
        self.near |= (np.abs(np.abs(raw) - self.law.lim) <= NEAR * self.law.lim).any(axis=1)
        return self.law.clamp(raw)


@pytest.mark.parametrize("name", CHAINS)
def test_no_evaluation_of_the_one_step_inputs_sits_at_a_limit(name):
    _, ref, _ = _trio(name, oracle=True)
    n = ref.n
    for integrator, hold in DIRECTIONAL_MODES:
        for per_sample in (False, True):
            near = total = 0
            for N in (1, 63, 64, 65, 200):
                q0, dq0, tau = _inputs(name, n, N, 1, seed=12100 + N)
                watch = _Watch(_law(name, n, N, 1, 12100 + N, per_sample, True, True, True, q0, dq0, tau), N)
                _np_closed_loop(_oracle_fd(ref), watch, q0, dq0, 1, DT, integrator, hold)
                near, total = near + int(watch.near.sum()), total + N
            print("%s %s hold=%d per_sample=%d: %d of %d samples within %g lim of a limit" % (name, integrator, hold, per_sample, near, total, NEAR))
            assert near <= 0.01 * total


@pytest.mark.parametrize("name", DIRECTIONAL_CHAINS)
def test_the_directional_table_is_what_the_oracle_measures(name):
    chain, ref, _ = _trio(name, oracle=True)
    for integrator, hold in DIRECTIONAL_MODES:
        got = _measure_directional(ref, name, integrator, hold, chain.getLinksNumber())
        for what, value in FB_DIRECTIONAL[(name, integrator, hold)].items():
            assert abs(got[what] - value) <= 0.05 * value, (integrator, hold, what, got[what], value)


@pytest.mark.parametrize("name", DIRECTIONAL_CHAINS)
def test_the_step_and_the_kept_share_of_the_directional_test_with_limits(name):
    chain, ref, _ = _trio(name, oracle=True)
    step, share, noise, clamped = _measure_limits(ref, name, chain.getLinksNumber())
    print("%s: step %g, kept share %.3f .. %.3f, %.1f %% of the commands clamped" % (name, step, min(share.values()), max(share.values()), 100 * clamped))
    assert step == FB_LIMIT_STEP[name] and min(share.values()) >= 0.5 and 0.2 <= clamped <= 0.8
    for integrator, _ in LIMIT_MODES:
        worst = max(v for (i, _), v in noise.items() if i == integrator)
        assert 0.5 * FB_LIMIT_NOISE[(name, integrator)] <= worst <= 2.0 * FB_LIMIT_NOISE[(name, integrator)], (integrator, worst)
