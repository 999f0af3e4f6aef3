"""CPU tests (no GPU): the premises of tests/test_gpu_rollout_feedback.py, from the oracle alone.  They are conditions on the tests' inputs,
not measurements of the device: the closed loop of the multi-step test is well enough conditioned that a bound of 8 dev means something,
the table of measured deviations is what the documented method gives, and the limits of the saturation test clamp a fair share of the
commands."""
import numpy as np
import pytest

from _arrays import INTEGRATORS
from _chains import WRENCH_CHAINS as CHAINS, _cpair
from _feedback import FB_MULTI_STEP, GAIN_FACTOR, _measure

MODES = [(integrator, hold) for integrator in INTEGRATORS for hold in ((True,) if integrator == "semi_implicit_euler" else (True, False))]


@pytest.mark.parametrize("name", CHAINS)
def test_the_oracle_alone_keeps_the_deviation_small_and_the_table_is_what_the_method_gives(name):
    """_feedback._measure: every ddq of the oracle's closed loop perturbed by 1e-11 relative; dev = the worst end-state deviation.  Below
    1e-9 at the recorded gain factor, and the row of FB_MULTI_STEP (the GPU tests' bound is 8 times it) is this measurement."""
    _, ref = _cpair(name)
    assert GAIN_FACTOR[name] in (1.0, 0.3, 0.1)
    for integrator, hold in MODES:
        dev = _measure(ref, name, integrator, hold)[0]
        row = FB_MULTI_STEP[(name, integrator, hold)]
        print("%s %s hold=%d: dev %.3g (table %.3g)" % (name, integrator, hold, dev, row))
        assert np.isfinite(dev) and dev < 1e-9, (integrator, hold, dev)
        assert abs(dev - row) <= 0.05 * row, (integrator, hold, dev, row)


@pytest.mark.parametrize("name", CHAINS)
def test_the_limits_clamp_between_a_fifth_and_four_fifths_of_the_commands(name):
    """the oracle's run of the multi-step inputs with the saturation test's limits: the share of (sample, joint, step) commands of the
    steps' first evaluations whose unclamped value lies outside the limit"""
    _, ref = _cpair(name)
    for integrator, hold in MODES:
        _, rec, _ = _measure(ref, name, integrator, hold, limits=True)
        raw, u = np.stack([r[2] for r in rec]), np.stack([r[3] for r in rec])
        share = float((raw != u).mean())
        print("%s %s hold=%d: %.1f %% of the commands are clamped" % (name, integrator, hold, 100 * share))
        assert 0.2 <= share <= 0.8, (integrator, hold, share)
