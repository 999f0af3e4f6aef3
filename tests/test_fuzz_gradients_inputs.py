"""What tests/test_gpu_fuzz_gradients.py rests on, pinned with the oracle alone (no GPU) on the committed fuzz seeds 1000 .. 1063: every
regular seed gets components, their friction joints see the linear band and the saturation, the run-time rollout bound with components is
finite and small, the components move the oracle's own forward dynamics and rollouts by more than the bounds the GPU tests assert (so
their "the components matter" assertions cannot be vacuous), the closed-form slopes are the oracle's, and the seeds reach what the
derivative, VJP and adjoint kernels had not seen: every register instance, permuted subsets with locked moveable joints, prismatic joints,
both layouts."""
import numpy as np
import pytest

from _arrays import INTEGRATORS, PRISMATIC, _inf
from _components import FRICTION1, FRICTION2, MAX_VELOCITY, MIN_VELOCITY, SPRING, _pin_the_closed_form_to_the_oracle
from _fuzz import FUZZ_OFFSET, case, rollout_bound, seed_class
from _references import _reference
import _fuzz as fg


@pytest.fixture(scope="module")
def regular():
    if FUZZ_OFFSET != 0:
        pytest.skip("the pinned facts are those of the committed seeds (RDYN_FUZZ_OFFSET=0)")
    cases = [c for c in (case(seed) for seed in range(64)) if c.full.n > 0]
    out = [c for c in cases if seed_class(c) == "regular"]
    assert len(out) == 58
    return out


def test_every_regular_seed_gets_components_scaled_to_its_lightest_joint(regular):
    for c in regular:
        specs = fg.fuzz_specs(c)
        s = fg.component_scale(c)
        d = np.einsum("sii->si", c.M).min()
        assert len(specs) >= 1 and len(specs) == {1: 3, 2: 4}.get(c.n, 5), (c.seed, c.n, len(specs))
        assert s > 0.0 and np.log2(s) == np.floor(np.log2(s)) and s <= d < 2.0 * s
        assert all(0 <= j < c.n for _, j, _, _, _ in specs)
        assert {ty for ty, _, _, _, _ in specs} == {FRICTION1, FRICTION2, SPRING}
        assert all(lo == (0.0 if ty == SPRING else MIN_VELOCITY) and hi == (0.0 if ty == SPRING else MAX_VELOCITY) for ty, _, lo, hi, _ in specs)
        assert specs[0][4] == (2.0 * s, 1.5 * s, 0.0)
    scales = [fg.component_scale(c) for c in regular]
    print("component scale s over the %d regular seeds: %.3g .. %.3g" % (len(regular), min(scales), max(scales)))


def test_the_friction_joints_see_the_linear_band_and_the_saturation(regular):
    pooled = np.concatenate([np.abs(c.dq[:, sorted({j for ty, j, _, _, _ in fg.fuzz_specs(c) if ty != SPRING})]).ravel() for c in regular])
    band, sat = float((pooled < MIN_VELOCITY).mean()), float((pooled > MAX_VELOCITY).mean())
    print("|dq| of the friction joints, %d entries pooled: %.1f %% below %.1f, %.1f %% above %.1f" % (pooled.size, 100 * band, MIN_VELOCITY, 100 * sat, MAX_VELOCITY))
    assert band >= 0.2 and sat >= 0.1, (band, sat)


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_the_run_time_rollout_bound_with_components_is_small_and_the_components_matter(regular, integrator):
    worst, least, fastest = 0.0, np.inf, 0.0
    for c in regular:
        bound, dev, qr, dqr = fg.rollout_bound_c(c, integrator)
        assert np.isfinite(bound) and 0.0 < bound < 1e-8, (c.seed, bound)
        assert np.isfinite(qr).all() and np.isfinite(dqr).all()
        worst = max(worst, dev)
        fastest = max(fastest, float(np.abs(dqr).max()))
        # the same oracle rollout without components: away from the one with them by more than the bound, on some sample
        _, _, qp, dqp = rollout_bound(c, integrator)
        scale = np.maximum(1.0, np.maximum(_inf(qr), _inf(dqr)))
        moved = float((np.maximum(_inf(qp - qr), _inf(dqp - dqr)) / scale).max())
        assert moved > bound, (c.seed, moved, bound)
        least = min(least, moved / bound)
    print("%s: perturbation deviation %.3g at the most (bound 8 x that, limit 1e-8); |dq| at the end <= %.3g; the components move the end "
          "state by %.3g bounds at the least" % (integrator, worst, fastest, least))


def test_the_components_move_the_forward_dynamics_residual_above_its_bound(regular):
    """c.tau = M_ref a + h_ref: the plain solution a leaves exactly tau_c_ref as its residual against h_ref + tau_c_ref"""
    least = np.inf
    for c in regular:
        tau_c = fg.component_torque_ref(c)
        scale = np.abs(c.M).sum(axis=2).max(axis=1) * _inf(c.a) + _inf(c.tau) + _inf(c.h) + _inf(tau_c)
        ratio = float((_inf(tau_c) / scale).max())
        assert ratio > 1e-11, (c.seed, ratio)
        least = min(least, ratio)
    print("the plain forward dynamics misses the residual with components by %.3g of the scale at the least (bound 1e-11)" % least)


def test_the_closed_form_slopes_are_the_oracle_s_on_the_fuzz_inputs(regular):
    for c in regular:
        _pin_the_closed_form_to_the_oracle(fg.fuzz_specs(c), c.n, c.q, c.dq)   # asserts its 5 % cap on the entries left out, too


def test_the_slopes_move_the_derivative_residuals_above_one_in_a_million(regular):
    """test_forward_dynamics_derivatives asserts that the residual without the slopes exceeds 1e-6.  Here the same ratio, in the units of
    _residual_ratios, for the oracle's exact X = -M_ref^-1 (D_ref + diag slopes) at the oracle's own ddq: the inputs allow the assertion."""
    from _components import _slopes
    from _references import _norm_inf
    least = {"dddq_dq": np.inf, "dddq_dv": np.inf}
    for c in regular:
        specs = fg.fuzz_specs(c)
        ddq = np.linalg.solve(c.M, (c.tau - c.h - fg.component_torque_ref(c))[:, :, None])[:, :, 0]
        Dq, Dv, tau_ref, _ = _reference(c.ref, c.oracle_types(), c.q, c.dq, ddq)
        idx = np.arange(c.n)
        mn = _norm_inf(c.M)
        for what, D, sl in (("dddq_dq", Dq, _slopes(specs, c.q, c.dq)[0]), ("dddq_dv", Dv, _slopes(specs, c.q, c.dq)[1])):
            full = D.copy()
            full[:, idx, idx] += sl
            X = -np.linalg.solve(c.M, full)
            ratio = float((_inf(np.einsum("sij,sjk->sik", c.M, X) + D) / (mn * _inf(X) + _inf(D) + _inf(tau_ref))).max())
            if c.n >= 2 or np.abs(sl).max() > 0.0:
                assert ratio > 1e-6, (c.seed, what, ratio)
                least[what] = min(least[what], ratio)
    print("residual without the slopes, exact X: dddq_dq %.3g dddq_dv %.3g at the least (must exceed 1e-6)" % (least["dddq_dq"], least["dddq_dv"]))


def test_the_seeds_reach_what_the_gradient_kernels_had_not_seen(regular):
    assert {c.ref.nJ for c in regular} == set(range(1, 11))                 # k_fwd_dyn_deriv / k_fwd_dyn_vjp / k_rollout_adjoint <1> .. <10>
    assert {3, 4, 5, 9} <= {c.ref.nJ for c in regular}                      # the instances no named chain gives
    assert set(range(1, 10)) <= {c.n for c in regular}
    locked = [c for c in regular if c.inputs is not None and len(c.inputs) < c.full.n]
    assert locked and any(c.inputs != [nm for nm in c.full.spec.moveable if nm in c.inputs] for c in locked)   # locked AND permuted
    assert any(c.ref.nJ > c.full.n for c in regular)                        # fixed joints inside the chain
    assert any(PRISMATIC in c.oracle_types() for c in regular) and any(c.oracle_types().count(PRISMATIC) >= 2 for c in regular)
    assert {c.layout for c in regular} == {"sample", "element"}
    print("%d regular seeds; %d subset seeds with a locked moveable joint; nJ %s" % (len(regular), len(locked), sorted({c.ref.nJ for c in regular})))
