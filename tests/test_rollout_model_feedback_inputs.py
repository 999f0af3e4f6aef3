"""CPU tests (no GPU): the premises of tests/test_gpu_rollout_model_feedback.py, from the oracle alone.  They are conditions on the tests'
inputs, not measurements of the device: the tables of measured deviations in tests/_model_feedback.py are what the documented methods
give, the limits of the saturation test clamp a fair share of the commands, and few samples have a command so close to a limit that the
comparison leaves them out."""
import numpy as np
import pytest

from _arrays import INTEGRATORS
from _chains import _cpair
from _model_feedback import (CHAINS, LAWS, LIMIT_FACTOR_CT, MF_CLOSED_FORM, MF_MULTI_STEP, SMALL_CHAINS, _measure_closed_form, _measure_model,
                             _near_a_limit)

MODES = [(integrator, hold) for integrator in INTEGRATORS for hold in ((True,) if integrator == "semi_implicit_euler" else (True, False))]


def test_the_tables_have_a_row_for_every_case_of_the_gpu_tests():
    assert set(MF_MULTI_STEP) == {(name, integrator, hold, law) for name in CHAINS for integrator, hold in MODES for law in LAWS}
    assert set(MF_CLOSED_FORM) == {(name, integrator) for name in CHAINS for integrator in INTEGRATORS}
    assert set(LIMIT_FACTOR_CT) == {(name, law) for name in CHAINS for law in LAWS}
    assert all(np.isfinite(v) and 0 < v < 1e-8 for v in list(MF_MULTI_STEP.values()) + list(MF_CLOSED_FORM.values()))


@pytest.mark.parametrize("name", SMALL_CHAINS)
@pytest.mark.parametrize("law", LAWS)
def test_the_multi_step_table_is_what_the_method_gives(name, law):
    """_model_feedback._measure_model: every ddq and every model torque of the oracle's closed loop perturbed by 1e-11 relative; the row of
    MF_MULTI_STEP (the GPU tests' bound is 8 times it) is this measurement, within the 5 % test_rollout_feedback_inputs.py allows."""
    _, ref = _cpair(name)
    for integrator, hold in MODES:
        dev = _measure_model(ref, name, integrator, hold, law)[0]
        row = MF_MULTI_STEP[(name, integrator, hold, law)]
        print("%s %s hold=%d %s: dev %.3g (table %.3g)" % (name, integrator, hold, law, dev, row))
        assert np.isfinite(dev) and abs(dev - row) <= 0.05 * row, (integrator, hold, dev, row)


@pytest.mark.parametrize("name", SMALL_CHAINS)
def test_the_closed_form_table_is_what_the_method_gives(name):
    """the oracle's own loop with the exact model against the 2 x 2 recurrence of the error dynamics: rounding alone, so the figure is
    pinned within a factor (it is a few ulp of the state) and has to be tiny"""
    _, ref = _cpair(name)
    for integrator in INTEGRATORS:
        dev, row = _measure_closed_form(ref, name, integrator), MF_CLOSED_FORM[(name, integrator)]
        print("%s %s: dev %.3g (table %.3g)" % (name, integrator, dev, row))
        assert abs(dev - row) <= 0.05 * row and dev < 1e-11, (integrator, dev, row)


@pytest.mark.parametrize("name", SMALL_CHAINS)
@pytest.mark.parametrize("law", LAWS)
def test_the_limits_clamp_a_fair_share_and_few_commands_sit_on_a_limit(name, law):
    """the oracle's run of the multi-step inputs with the saturation test's limits: between 20 % and 80 % of the (sample, joint, step)
    commands of the steps' first evaluations are clamped, and at most 5 % of the samples have a raw command within the law's rounding of
    a limit"""
    _, ref = _cpair(name)
    for integrator, hold in MODES:
        _, rec, _, l = _measure_model(ref, name, integrator, hold, law, limits=True)
        raw, u = np.stack([r[2] for r in rec]), np.stack([r[3] for r in rec])
        share, near = float((raw != u).mean()), float(_near_a_limit(rec, l).mean())
        print("%s %s hold=%d %s: %.1f %% clamped, %.1f %% of the samples near a limit" % (name, integrator, hold, law, 100 * share, 100 * near))
        assert 0.2 <= share <= 0.8, (integrator, hold, share)
        assert near <= 0.05, (integrator, hold, near)
