"""GPU tests of rdyn_forward_dynamics_vjp / Chain.getJointAccelerationVjp: with ddq = FD_c(q, dq, tau) and a seed a on ddq
    tau_bar = M^-1 a,   q_bar = dddq_dq' a = -(dtau_dq + diag d tau_c / d q)' tau_bar,   dq_bar = dddq_dv' a = -(dtau_dv + diag d tau_c / d dq)' tau_bar,
dtau_dq, dtau_dv the derivatives of the joint torque at that very ddq.

Oracle, residual form (every sample, none excused).  With ddq the call's own output, M_ref the oracle's inertia, D_ref the exact spectral /
central-difference derivative of the oracle torque at that ddq (test_gpu_torque_derivatives.py; its 8-against-16-point gap is asserted
<= 1e-12 of its scale) and tau_ref the oracle torque there:
    |M_ref tau_bar - a|_inf          <= 1e-11 (|M_ref|_inf |tau_bar|_inf + |a|_inf)
    |q_bar  + Dq_ref' tau_bar|_inf   <= 1e-11 gscale |tau_bar|_1       gscale = max(|Dq_ref|_inf, |Dv_ref|_inf) + |tau_ref|_inf
    |dq_bar + Dv_ref' tau_bar|_inf   <= 1e-11 gscale |tau_bar|_1
1e-11 is the project's parity figure for M and D; the residual form keeps cond(M) out of the bound.  Components: the same residuals with
the closed-form slopes of test_gpu_forward_dynamics_derivatives.py (_slopes, pinned there to oracle/components_oracle.c) on the
diagonals of D_ref."""
import numpy as np
import pytest

from _arrays import VJP_NAMES as NAMES, _dev, _host, _inputs, _seed, _vjp_call as _call
from _chains import GRAV, _chain, _pair
from _components import MAX_VELOCITY, MIN_VELOCITY, _set, _slopes, _specs
from _references import _cached_reference, _input_types, _vjp_residual_ratios as _residual_ratios

pytestmark = pytest.mark.gpu
ORACLE_CHAINS = ["planar_2r", "rev1", "mixed_joints", "ur10_public", "panda_like", "ur10_public_long", "rev8", "rev10", "rev14",
                 "gen20_permuted", "rev32"]
SIZES = (1, 63, 64, 65, 200)


# ---- 1. the oracle, residual form
@pytest.mark.parametrize("layout", ["sample", "element"])
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("name", ORACLE_CHAINS)
def test_against_the_oracle_in_residual_form(name, N, layout):
    torch = pytest.importorskip("torch")
    chain, ref = _pair(name)
    n = ref.n
    q, dq, tau = _inputs(n, N)
    a = _seed(n, N)
    st, qb, vb, tb, ddq = _call(torch, chain, q, dq, tau, a, layout)
    assert st.shape == (N,) and (st == 1).all(), np.unique(st)
    assert all(x.shape == (N, n) and np.isfinite(x).all() for x in (qb, vb, tb, ddq))
    plain, st2 = chain.getJointAcceleration(_dev(torch, q, layout), _dev(torch, dq, layout), _dev(torch, tau, layout), layout=layout)
    assert np.array_equal(_host(plain, layout), ddq) and (st2.cpu().numpy() == 1).all()
    worst = _residual_ratios(_cached_reference((name, N, 0), ref, _input_types(chain), q, dq, ddq), a, qb, vb, tb)
    print("%s %s N=%d: worst residual ratio tau_bar %.3g q_bar %.3g dq_bar %.3g (bound 1e-11)"
          % (name, layout, N, worst["tau_bar"], worst["q_bar"], worst["dq_bar"]))
    for what, r in worst.items():
        assert r <= 1e-11, (what, r)


# ---- 2. components
@pytest.mark.parametrize("name", ["ur10_public", "mixed_joints", "rev10", "rev14"])
def test_components_put_their_slopes_into_the_products(name):
    torch = pytest.importorskip("torch")
    chain, ref = _pair(name)
    n, N = ref.n, 200
    specs = _specs(n)
    cs = _set(specs, n)
    q, dq, tau = _inputs(n, N, seed=4100)
    a = _seed(n, N, seed=4100)
    band, sat = (np.abs(dq) < MIN_VELOCITY).mean(), (np.abs(dq) > MAX_VELOCITY).mean()
    assert 0.2 < band < 0.4 and 0.1 < sat < 0.3, (band, sat)
    for layout in ("sample", "element"):
        st, qb, vb, tb, ddq = _call(torch, chain, q, dq, tau, a, layout, components=cs)
        assert (st == 1).all()
        want, _ = chain.getJointAcceleration(_dev(torch, q, layout), _dev(torch, dq, layout), _dev(torch, tau, layout), layout=layout, components=cs)
        assert np.array_equal(_host(want, layout), ddq)
        cached = _cached_reference((name, N, 1), ref, _input_types(chain), q, dq, ddq)
        worst = _residual_ratios(cached, a, qb, vb, tb, slopes=_slopes(specs, q, dq))
        print("%s %s with components: worst residual ratio tau_bar %.3g q_bar %.3g dq_bar %.3g (bound 1e-11)"
              % (name, layout, worst["tau_bar"], worst["q_bar"], worst["dq_bar"]))
        for what, r in worst.items():
            assert r <= 1e-11, (what, r)
        # the slopes matter at this bound: without them the residual is far off
        bare = _residual_ratios(cached, a, qb, vb, tb)
        assert bare["q_bar"] > 1e-6 and bare["dq_bar"] > 1e-6, bare
        # an empty list is the plain call, bitwise
        x = _call(torch, chain, q, dq, tau, a, layout, components=_set([], n))
        y = _call(torch, chain, q, dq, tau, a, layout)
        for u, v in zip(x, y):
            assert np.array_equal(u, v)


# ---- 3. failure statuses
@pytest.mark.parametrize("layout", ["sample", "element"])
def test_inertia_that_is_not_positive_definite_reports_minus_one_and_nan(layout):
    """ur10_public with the fixed joint of tool0 among the input joints: its row and column of M are zero."""
    import os
    torch = pytest.importorskip("torch")
    from conftest import FIXTURES
    from rosdyn_amd import Chain
    chain = Chain(os.path.join(FIXTURES, "ur10_public.urdf"), "base_link", "tool0", GRAV)
    moving = ["shoulder_pan_joint", "shoulder_lift_joint", "elbow_joint", "wrist_1_joint", "wrist_2_joint", "wrist_3_joint"]
    assert chain.setInputJointsName(moving[:3] + ["flange-tool0"] + moving[3:])
    n, N = 7, 200
    q, dq, tau = _inputs(n, N, seed=33)
    out = _call(torch, chain, q, dq, tau, _seed(n, N, seed=33), layout)
    assert (out[0] == -1).all() and all(np.isnan(x).all() for x in out[1:])


@pytest.mark.parametrize("name", ["ur10_public", "rev10", "rev14"])
@pytest.mark.parametrize("layout", ["sample", "element"])
def test_a_nan_in_one_seed_fails_that_sample_alone(name, layout):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 200
    q, dq, tau = _inputs(n, N, seed=35)
    a = _seed(n, N, seed=35)
    clean = _call(torch, chain, q, dq, tau, a, layout)
    assert (clean[0] == 1).all()
    for bad, value in ((70, np.nan), (3, np.inf)):
        b = a.copy()
        b[bad, n // 2] = value
        got = _call(torch, chain, q, dq, tau, b, layout)
        others = np.arange(N) != bad
        assert got[0][bad] == -1 and (got[0][others] == 1).all()
        for x, y in zip(got[1:], clean[1:]):
            assert np.isnan(x[bad]).all() and np.array_equal(x[others], y[others])
    # ... and so does a non-finite state or torque
    for which in range(3):
        args = [q.copy(), dq.copy(), tau.copy()]
        args[which][129, 0] = np.nan
        got = _call(torch, chain, args[0], args[1], args[2], a, layout)
        others = np.arange(N) != 129
        assert got[0][129] == -1 and (got[0][others] == 1).all()
        for x, y in zip(got[1:], clean[1:]):
            assert np.isnan(x[129]).all() and np.array_equal(x[others], y[others])


# ---- 4. aliasing and optional outputs
@pytest.mark.parametrize("name", ["panda_like", "rev10", "gen20_permuted"])
def test_layouts_subsets_and_the_aliased_seed_agree_bitwise(name):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 200
    q, dq, tau = _inputs(n, N, seed=4400)
    a = _seed(n, N, seed=4400)
    full = _call(torch, chain, q, dq, tau, a, "sample")
    assert (full[0] == 1).all()
    el = _call(torch, chain, q, dq, tau, a, "element")
    for x, y in zip(full, el):
        assert np.array_equal(x, y)
    every = NAMES + ("ddq",)
    for layout in ("sample", "element"):
        for mask in range(1, 16):
            want = tuple(k for b, k in enumerate(every) if mask >> b & 1)
            if want == ("ddq",):
                continue
            part = _call(torch, chain, q, dq, tau, a, layout, want=want)
            assert np.array_equal(part[0], full[0])
            for k, t in zip(want, part[1:]):
                assert np.array_equal(t, full[1 + every.index(k)]), (layout, want, k)
        # tau_bar written over the seed, alone and with the other products
        for want in (("tau",), NAMES):
            ta = _dev(torch, a, layout)
            out = chain.getJointAccelerationVjp(_dev(torch, q, layout), _dev(torch, dq, layout), _dev(torch, tau, layout), ta, layout=layout,
                                                want=want, out={"tau": ta})
            assert out[1 + want.index("tau")].data_ptr() == ta.data_ptr()
            for k, t in zip(want, out[1:]):
                assert np.array_equal(_host(t, layout), full[1 + every.index(k)]), (layout, want, k)


def test_chunk_size_does_not_change_the_result():
    torch = pytest.importorskip("torch")
    chain = _chain("rev14")
    n, N = 14, 200
    q, dq, tau = _inputs(n, N, seed=21)
    a = _seed(n, N, seed=21)
    x = _call(torch, chain, q, dq, tau, a, "sample")
    y = _call(torch, chain, q, dq, tau, a, "sample", chunk_samples=64)
    z = _call(torch, chain, q, dq, tau, a, "element", chunk_samples=70)
    assert (x[0] == 1).all()
    for u, v, w in zip(x, y, z):
        assert np.array_equal(u, v) and np.array_equal(u, w)
