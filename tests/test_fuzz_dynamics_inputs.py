"""What tests/test_gpu_fuzz_dynamics.py rests on, pinned with the oracle alone (no GPU): the committed fuzz seeds 1000 .. 1063 classify into
regular and singular chains with nothing in between, they reach every kernel instance and the subset path, the exact derivative reference
passes its own construction check, and the run-time rollout bound is finite and small."""
import numpy as np
import pytest

from _arrays import INTEGRATORS, PRISMATIC, _inf
from _fuzz import FUZZ_OFFSET, REGULAR_LAMBDA, case, reference_derivatives, rollout_bound, seed_class

SINGULAR_SEEDS = {0, 8, 21, 22, 60}


@pytest.fixture(scope="module")
def cases():
    if FUZZ_OFFSET != 0:
        pytest.skip("the pinned facts are those of the committed seeds (RDYN_FUZZ_OFFSET=0)")
    return [c for c in (case(seed) for seed in range(64)) if c.full.n > 0]


def test_every_seed_classifies_and_the_singular_seeds_are_the_known_five(cases):
    assert sorted(set(range(64)) - {c.seed for c in cases}) == [38]        # the one sub-path without a moveable joint
    kinds = {c.seed: seed_class(c) for c in cases}                       # asserts: no sample in neither class, no mixed seed
    assert {s for s, k in kinds.items() if k == "singular"} == SINGULAR_SEEDS
    lam = min(c.lam.min() for c in cases if kinds[c.seed] == "regular")
    print("regular seeds: lambda_min(M_ref) / trace(M_ref) >= %.3g (class boundary %.0e)" % (lam, REGULAR_LAMBDA))
    assert lam >= REGULAR_LAMBDA
    regular = [c for c in cases if kinds[c.seed] == "regular"]
    print("regular seeds: |h_ref| <= %.3g, |tau| <= %.3g (forward dynamics), %.3g (rollouts)"
          % (max(np.abs(c.h).max() for c in regular), max(np.abs(c.tau).max() for c in regular), max(np.abs(c.tau_seq).max() for c in regular)))
    assert all(np.isfinite(c.tau).all() and np.isfinite(c.tau_seq).all() for c in regular)


def test_the_seeds_reach_every_kernel_instance_and_the_subset_path(cases):
    assert {c.ref.nJ for c in cases} == set(range(1, 11))                   # k_fwd_dyn / k_torque_deriv / k_rollout <1> .. <10>
    assert {c.ref.nJ for c in cases if c.regular.all()} == set(range(1, 11))
    assert set(range(1, 10)) <= {c.n for c in cases}
    subsets = [c for c in cases if c.inputs is not None]
    assert len(subsets) >= 25
    assert any(len(c.inputs) < c.full.n for c in subsets if c.regular.all())   # a moveable joint that is not an input joint
    assert any(PRISMATIC in c.oracle_types() for c in cases) and any(c.ref.nJ > c.full.n for c in cases)   # prismatic, fixed joints
    assert {c.layout for c in cases} == {"sample", "element"}


def test_the_spectral_reference_passes_its_construction_check_on_every_seed(cases):
    worst = 0.0
    for c in cases:
        Dq, Dv, tau, gap = reference_derivatives(c)
        scale = np.maximum(_inf(Dq), _inf(Dv)) + _inf(tau)
        assert (gap <= 1e-12 * scale).all(), (c.seed, float((gap / scale).max()))
        worst = max(worst, float((gap / np.maximum(scale, np.finfo(np.float64).tiny)).max()))
    print("construction gap, 8 against 16 points: %.3g of the scale at the most (bound 1e-12)" % worst)


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_the_run_time_rollout_bound_is_finite_and_small_on_every_regular_seed(cases, integrator):
    worst = 0.0
    for c in cases:
        if not c.regular.all():
            continue
        bound, dev, qr, dqr = rollout_bound(c, integrator)
        assert np.isfinite(bound) and 0.0 < bound < 1e-8, (c.seed, bound)
        assert np.isfinite(qr).all() and np.isfinite(dqr).all()
        worst = max(worst, bound)
    print("%s: run-time rollout bound %.3g at the most (limit 1e-8)" % (integrator, worst))
