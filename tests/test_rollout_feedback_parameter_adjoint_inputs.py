"""CPU tests (no GPU, the oracle alone) of the premises of the central-difference tests of the closed loop's parameter gradient
(tests/test_gpu_rollout_feedback_parameter_adjoint.py, tests 6 and 7; _feedback_parameters.py has the setting and the method, which is
that of tests/test_parameter_gradient_inputs.py with the closed loop of _feedback.py in place of the open rollout).

Without limits: every recorded worst err(H) / scale (FBP_ORACLE_WORST) is re-measured within 5 %, and at least three quarters of the
samples qualify (err(H) >= 1e-9 scale), so that the ratio test on the device has its samples.
With limits under hold = 1: the step (FBP_LIMIT_STEP) is the largest of 1e-1, 1e-2, 1e-3 at which the oracle keeps at least half of the
samples under both integrators; the recorded noise figures (FBP_LIMIT_NOISE) are re-measured within 5 %; 20 - 80 % of the commands of the
unperturbed run are clamped.
`python tests/test_rollout_feedback_parameter_adjoint_inputs.py` prints the tables."""
import pytest

from _feedback_parameters import (CD_CHAINS, FBP_LIMIT_NOISE, FBP_LIMIT_STEP, FBP_ORACLE_WORST, LIMIT_MODES, MODES, measure_limits, measure_smooth)


@pytest.mark.parametrize("mode", MODES, ids=["euler", "rk4-hold", "rk4-continuous"])
@pytest.mark.parametrize("name", CD_CHAINS)
def test_the_samples_qualify_and_the_error_is_what_was_recorded(name, mode):
    integrator, hold = mode
    r = measure_smooth(name, integrator, hold)
    qualify = int((r >= 1e-9).sum())
    recorded = FBP_ORACLE_WORST[(name, integrator, bool(hold))]
    print("%s %s hold %d: worst err(H) / scale %.3g (recorded %.3g), %d of %d samples qualify" % (name, integrator, hold, r.max(), recorded, qualify, len(r)))
    assert 4 * qualify >= 3 * len(r), qualify
    assert abs(r.max() / recorded - 1.0) <= 0.05, (float(r.max()), recorded)


@pytest.mark.parametrize("name", CD_CHAINS)
def test_the_step_with_limits_and_its_noise_are_what_was_recorded(name):
    step, share, noise, clamped = measure_limits(name)
    print("%s: step %g, kept %s, noise %s, %.1f %% of the commands clamped" % (name, step, share, noise, 100.0 * clamped))
    assert step == FBP_LIMIT_STEP[name]
    assert 0.2 <= clamped <= 0.8, clamped
    for integrator, _ in LIMIT_MODES:
        assert share[integrator] >= 0.5, (integrator, share[integrator])
        recorded = FBP_LIMIT_NOISE[(name, integrator)]
        assert abs(noise[integrator] / recorded - 1.0) <= 0.05, (integrator, noise[integrator], recorded)


if __name__ == "__main__":
    print("FBP_ORACLE_WORST = {")
    for name in CD_CHAINS:
        for integrator, hold in MODES:
            r = measure_smooth(name, integrator, hold)
            print("    (%r, %r, %r): %.3e,   # %d of %d qualify" % (name, integrator, bool(hold), r.max(), int((r >= 1e-9).sum()), len(r)))
    print("}")
    for name in CD_CHAINS:
        step, share, noise, clamped = measure_limits(name)
        print("%s: step %g kept %s clamped %.3f" % (name, step, share, clamped))
        for integrator, _ in LIMIT_MODES:
            print("    (%r, %r): %.3e," % (name, integrator, noise[integrator]))
