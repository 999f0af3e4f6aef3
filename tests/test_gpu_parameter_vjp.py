"""GPU tests of rdyn_forward_dynamics_parameter_vjp / Chain.getJointAccelerationParameterVjp and of Chain.withParameters on the device:
with ddq = FD_c(q, dq, tau), a seed a on ddq and tau_bar = M^-1 a
    pi_bar = -Y(q, dq, ddq)' tau_bar        comp_bar = -C(q, dq)' tau_bar.

Reference: Y_ref = the CPU oracle's regressor evaluated AT THE LIBRARY'S OWN ddq (cond(M) stays out of the bound), tau_bar_lib from
getJointAccelerationVjp, C from rdyn_components_regressor.  Bound per entry: 1e-11 (the project's parity figure) times the sum of the
absolute values of the entry's terms, |Y_ref|' |tau_bar|; the worst ratio is printed.  Sums: 1e-12 sum |rows| (N eps with room).
That plain bound is asserted on every entry but the RESIDUE entries of Y_ref: where an entry of Y_ref is itself what rounding leaves of
terms that cancel, 1e-11 of it bounds nothing an implementation could meet -- the oracle of mixed_joints has 2.8e-17 in the Ixz column
of a link that turns about its z axis, beside 1.0 in Izz; that of panda_like 8.9e-16 in a first-moment column beside 14.5 in the same row
of the same link; the true value is 0.  An entry is residue when the sum of its absolute terms is at most RESIDUE = 64 eps of its link
block's scale (the largest |Y_ref| of the block times |tau_bar|_1): the ten columns of a link are made of the same few kinematic vectors
rotated into its frame, and a sum below a few roundings of the largest of them cannot be told from rounding.  Measured on the oracle with
the device's rows: the two kinds are fifteen orders apart (residue entries at most 0.006 eps of the scale, every other non-zero entry at
least 3e7 eps).  Residue entries are held to 8 eps of that scale instead (measured: 0.007 eps).
Sizes 1, 63, 65, 130: one lane, a partial wave, the wave boundary, three waves.
rev14 takes the chunked route (more than 10 input joints): its rows and sums do not depend on chunk_samples."""
import numpy as np
import pytest

from _arrays import _dev, _host, _inputs, _seed
from _chains import _cpair
from _components import MAX_VELOCITY, MIN_VELOCITY, _set, _specs

pytestmark = pytest.mark.gpu
CHAINS = ["planar_2r", "ur10_public", "mixed_joints", "panda_like", "ur10_permuted", "rev10", "ur10_public_long", "rev14"]
RESIDUE = 64.0 * np.finfo(np.float64).eps
SIZES = (1, 63, 65, 130)


def _call(torch, chain, q, dq, tau, a, layout, **kw):
    """host arrays: pi_bar, comp_bar (rows (N, cols), or sums), tau_bar (N, n), ddq (N, n), status (N,)"""
    out = chain.getJointAccelerationParameterVjp(_dev(torch, q, layout), _dev(torch, dq, layout), _dev(torch, tau, layout),
                                                 _dev(torch, a, layout), layout=layout, **kw)
    rows = not kw.get("reduce", False)
    pi, comp = ((_host(t, layout) if rows else t.cpu().numpy()) if t is not None else None for t in out[:2])
    return pi, comp, _host(out[2], layout), _host(out[3], layout), out[4].cpu().numpy()


def _vjp(torch, chain, q, dq, tau, a, layout, **kw):
    st, tb, ddq = chain.getJointAccelerationVjp(_dev(torch, q, layout), _dev(torch, dq, layout), _dev(torch, tau, layout),
                                                _dev(torch, a, layout), layout=layout, want=("tau", "ddq"), **kw)
    return _host(tb, layout), _host(ddq, layout), st.cpu().numpy()


_YREF = {}


def _y_ref(name, N, ref, q, dq, ddq):
    """the oracle's regressor at the library's ddq, once per (chain, N): shared by the layouts and the tests, read-only"""
    key = (name, N)
    if key not in _YREF:
        Y = ref.regressor(q, dq, ddq)
        Y.setflags(write=False)
        _YREF[key] = (ddq.copy(), Y)
    assert np.array_equal(_YREF[key][0], ddq), "the layouts must give the same ddq bits"
    return _YREF[key][1]


def _bound(Y, tb):
    """per entry (N, P): 1e-11 |Y_ref|' |tau_bar|, the issue's bound -- but for the residue entries of Y_ref (the module docstring), which
    get 8 eps of their link block's scale; returns (bound, residue mask)"""
    A, t = np.abs(Y), np.abs(tb)
    terms = np.einsum("snp,sn->sp", A, t)
    scale = np.repeat(A.reshape(A.shape[0], A.shape[1], -1, 10).max(axis=(1, 3)), 10, axis=1) * t.sum(axis=1)[:, None]
    residue = terms <= RESIDUE * scale
    return np.where(residue, 8.0 * np.finfo(np.float64).eps * scale, 1e-11 * terms), residue


# ---- 1. rows against the oracle's regressor; 3. the sibling's outputs bitwise
@pytest.mark.parametrize("layout", ["sample", "element"])
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("name", CHAINS)
def test_rows_against_the_oracle_regressor_at_the_librarys_ddq(name, N, layout):
    torch = pytest.importorskip("torch")
    chain, ref = _cpair(name)
    n = ref.n
    q, dq, tau = _inputs(n, N)
    a = _seed(n, N)
    pi, comp, tb, ddq, st = _call(torch, chain, q, dq, tau, a, layout)
    assert comp is None and pi.shape == (N, 10 * chain.getJointsNumber()) and (st == 1).all()
    tb2, ddq2, st2 = _vjp(torch, chain, q, dq, tau, a, layout)
    assert np.array_equal(tb, tb2) and np.array_equal(ddq, ddq2) and np.array_equal(st, st2)
    Y = _y_ref(name, N, ref, q, dq, ddq)
    want = -np.einsum("snp,sn->sp", Y, tb)
    bound, residue = _bound(Y, tb)
    err = np.abs(pi - want)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    terms = np.einsum("snp,sn->sp", np.abs(Y), np.abs(tb))
    print("%s %s N=%d: worst |pi_bar - ref| / sum |terms| %.3g (bound 1e-11) over %d entries; %d residue entries, worst error / (8 eps scale) %.3g"
          % (name, layout, N, (err[~residue] / terms[~residue]).max(), int((~residue).sum()), int(residue.sum()),
             ratio[residue].max() if residue.any() else 0.0))
    assert (~residue).sum() >= residue.sum() // 2 and (err <= bound).all(), (float(ratio.max()), np.unravel_index(np.argmax(ratio), ratio.shape))


# ---- 2. components
@pytest.mark.parametrize("layout", ["sample", "element"])
@pytest.mark.parametrize("name", ["ur10_public", "mixed_joints", "ur10_permuted", "rev10", "ur10_public_long", "rev14"])
def test_component_columns_against_the_component_regressor(name, layout):
    """_specs: two friction components and a spring on joint 0 (list order), a FRICTION2 on the last joint, a spring on joint 1; Dq in +-1
    against max_velocity 0.8: a fifth of the entries saturated, a third inside the linear band"""
    torch = pytest.importorskip("torch")
    chain, ref = _cpair(name)
    n, N = ref.n, 130
    cs = _set(_specs(n), n)
    q, dq, tau = _inputs(n, N, seed=4100)
    a = _seed(n, N, seed=4100)
    band, sat = (np.abs(dq) < MIN_VELOCITY).mean(), (np.abs(dq) > MAX_VELOCITY).mean()
    assert 0.2 < band < 0.4 and 0.1 < sat < 0.3, (band, sat)
    pi, comp, tb, ddq, st = _call(torch, chain, q, dq, tau, a, layout, components=cs)
    assert (st == 1).all() and comp.shape == (N, cs.columns)
    tb2, ddq2, st2 = _vjp(torch, chain, q, dq, tau, a, layout, components=cs)
    assert np.array_equal(tb, tb2) and np.array_equal(ddq, ddq2) and np.array_equal(st, st2)
    Cm = cs.getRegressor(_dev(torch, q, "sample"), _dev(torch, dq, "sample")).cpu().numpy()  # (N, K, n)
    want = -np.einsum("skn,sn->sk", Cm, tb)
    bound = 1e-11 * np.einsum("skn,sn->sk", np.abs(Cm), np.abs(tb))
    assert (np.abs(comp - want) <= bound).all(), float(np.abs(comp - want).max())
    assert np.abs(want).max() > 1e-3
    # the inertial rows with components: the same reference at this call's ddq
    Y = ref.regressor(q, dq, ddq)
    assert (np.abs(pi + np.einsum("snp,sn->sp", Y, tb)) <= _bound(Y, tb)[0]).all()
    # an empty list is the plain call, bitwise
    x = _call(torch, chain, q, dq, tau, a, layout, components=_set([], n))
    y = _call(torch, chain, q, dq, tau, a, layout)
    assert x[1] is None and all(np.array_equal(u, v) for u, v in zip(x[:1] + x[2:], y[:1] + y[2:]))


# ---- 4. sums
@pytest.mark.parametrize("layout", ["sample", "element"])
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("name", ["ur10_public", "rev10", "ur10_public_long", "rev14"])
def test_sums_equal_the_summed_rows_are_reproducible_and_accumulate(name, N, layout):
    torch = pytest.importorskip("torch")
    chain, _ = _cpair(name, oracle=False)
    n = chain.getActiveJointsNumber()
    cs = _set(_specs(n), n)
    q, dq, tau = _inputs(n, N, seed=52)
    a = _seed(n, N, seed=52)
    pi, comp, tb, ddq, st = _call(torch, chain, q, dq, tau, a, layout, components=cs)
    assert (st == 1).all()
    spi, scomp, tb2, ddq2, st2 = _call(torch, chain, q, dq, tau, a, layout, components=cs, reduce=True)
    assert np.array_equal(tb, tb2) and np.array_equal(ddq, ddq2) and np.array_equal(st, st2)
    for rows, s in ((pi, spi), (comp, scomp)):
        err, bound = np.abs(s - rows.sum(axis=0)), 1e-12 * np.abs(rows).sum(axis=0)
        print("%s %s N=%d: worst sum error / sum |rows| %.3g (bound 1e-12)" % (name, layout, N, (err / np.where(bound > 0, bound, 1e-12)).max() * 1e-12))
        assert (err <= bound).all()
    if N == 1:
        assert np.array_equal(spi, pi[0]) and np.array_equal(scomp, comp[0])
    again = _call(torch, chain, q, dq, tau, a, layout, components=cs, reduce=True)
    assert np.array_equal(again[0], spi) and np.array_equal(again[1], scomp)
    # accumulate = 1 adds to what is there
    base = (torch.full((spi.size,), 2.5, dtype=torch.float64, device="cuda"), torch.full((scomp.size,), -1.25, dtype=torch.float64, device="cuda"))
    chain.getJointAccelerationParameterVjp(_dev(torch, q, layout), _dev(torch, dq, layout), _dev(torch, tau, layout), _dev(torch, a, layout),
                                           components=cs, layout=layout, reduce=True, accumulate=base)
    assert np.array_equal(base[0].cpu().numpy(), 2.5 + spi) and np.array_equal(base[1].cpu().numpy(), -1.25 + scomp)


# ---- 5. failures
@pytest.mark.parametrize("layout", ["sample", "element"])
@pytest.mark.parametrize("name", ["ur10_public", "rev10", "ur10_public_long", "rev14"])
def test_a_nan_seed_fails_its_sample_alone_and_leaves_the_sums(name, layout):
    torch = pytest.importorskip("torch")
    chain, _ = _cpair(name, oracle=False)
    n, N, bad = chain.getActiveJointsNumber(), 130, 70
    cs = _set(_specs(n), n)
    q, dq, tau = _inputs(n, N, seed=35)
    a = _seed(n, N, seed=35)
    clean = _call(torch, chain, q, dq, tau, a, layout, components=cs)
    b = a.copy()
    b[bad, n // 2] = np.nan
    got = _call(torch, chain, q, dq, tau, b, layout, components=cs)
    others = np.arange(N) != bad
    assert got[4][bad] == -1 and (got[4][others] == 1).all()
    for x, y in zip(got[:4], clean[:4]):
        assert np.isnan(x[bad]).all() and np.array_equal(x[others], y[others])
    # the sums: those of the batch without the sample (the sample's place taken by a zero seed, whose rows are +-0)
    sums = _call(torch, chain, q, dq, tau, b, layout, components=cs, reduce=True)
    z = a.copy()
    z[bad] = 0.0
    without = _call(torch, chain, q, dq, tau, z, layout, components=cs, reduce=True)
    assert np.isfinite(sums[0]).all() and np.isfinite(sums[1]).all()
    assert np.array_equal(sums[0], without[0]) and np.array_equal(sums[1], without[1])
    for rows, s in ((clean[0], sums[0]), (clean[1], sums[1])):
        assert (np.abs(s - rows[others].sum(axis=0)) <= 1e-12 * np.abs(rows[others]).sum(axis=0)).all()


@pytest.mark.parametrize("layout", ["sample", "element"])
def test_an_indefinite_inertia_gives_nan_rows_and_zero_sums(layout):
    """the fixture of test_gpu_forward_dynamics_vjp.py: ur10_public with the fixed joint of tool0 among the input joints"""
    import os
    torch = pytest.importorskip("torch")
    from conftest import FIXTURES
    from rosdyn_amd import Chain
    from _chains import GRAV
    chain = Chain(os.path.join(FIXTURES, "ur10_public.urdf"), "base_link", "tool0", GRAV)
    moving = ["shoulder_pan_joint", "shoulder_lift_joint", "elbow_joint", "wrist_1_joint", "wrist_2_joint", "wrist_3_joint"]
    assert chain.setInputJointsName(moving[:3] + ["flange-tool0"] + moving[3:])
    n, N = 7, 130
    q, dq, tau = _inputs(n, N, seed=33)
    a = _seed(n, N, seed=33)
    pi, comp, tb, ddq, st = _call(torch, chain, q, dq, tau, a, layout)
    assert (st == -1).all() and all(np.isnan(x).all() for x in (pi, tb, ddq))
    spi = _call(torch, chain, q, dq, tau, a, layout, reduce=True)[0]
    assert (spi == 0.0).all()


# ---- 6. more input joints than the kernels sweep
def test_chunk_size_does_not_change_the_result():
    torch = pytest.importorskip("torch")
    import ctypes as C
    from rosdyn_amd._lib import lib
    chain, _ = _cpair("rev14", oracle=False)
    n, N = 14, 200
    cs = _set(_specs(n), n)
    q, dq, tau = _inputs(n, N, seed=21)
    a = _seed(n, N, seed=21)
    P, K = 10 * chain.getJointsNumber(), cs.columns
    comps, n_comps = chain._component_list(cs)

    def run(layout, chunk):
        t = [_dev(torch, x, layout) for x in (q, dq, tau, a)]
        b, _, lay = chain._batch(layout, t[0], t[1])
        shape = (lambda k: (N, k)) if layout == "sample" else (lambda k: (k, N))
        out = [torch.zeros(shape(k), dtype=torch.float64, device="cuda") for k in (P, K, n, n)]
        sums = [torch.zeros((k,), dtype=torch.float64, device="cuda") for k in (P, K)]
        st = torch.zeros((N,), dtype=torch.int32, device="cuda")
        nbytes = lib().rdyn_forward_dynamics_parameter_vjp_workspace_bytes(chain._h, comps, n_comps, N, chunk)
        assert nbytes > 0
        ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
        from rosdyn_amd._lib import check
        check(lib().rdyn_forward_dynamics_parameter_vjp(chain._h, C.byref(b), comps, n_comps, t[2].data_ptr(), t[3].data_ptr(), out[0].data_ptr(),
                                                        out[1].data_ptr(), sums[0].data_ptr(), sums[1].data_ptr(), 0, out[2].data_ptr(),
                                                        out[3].data_ptr(), st.data_ptr(), chunk, ws.data_ptr(), nbytes))
        return [_host(x, layout) for x in out] + [x.cpu().numpy() for x in sums] + [st.cpu().numpy()]

    x = run("sample", 0)
    assert (x[6] == 1).all() and np.abs(x[0]).max() > 0 and np.abs(x[1]).max() > 0
    for layout, chunk in (("sample", 64), ("sample", 70), ("element", 70), ("element", 0)):
        y = run(layout, chunk)
        assert all(np.array_equal(u, v) for u, v in zip(x, y)), (layout, chunk)
    # the sums alone (the rows then live in the workspace), and what the Python method returns
    s = _call(torch, chain, q, dq, tau, a, "sample", components=cs, reduce=True)
    assert np.array_equal(s[0], x[4]) and np.array_equal(s[1], x[5])


# ---- 7. through withParameters
@pytest.mark.parametrize("name", CHAINS)
def test_the_torque_of_a_chain_with_other_parameters_is_the_regressor_times_them(name):
    torch = pytest.importorskip("torch")
    chain, _ = _cpair(name, oracle=False)
    n, N = chain.getActiveJointsNumber(), 130
    pi0 = chain.getNominalParameters()
    pi1 = pi0 * (1.0 + 0.1 * np.random.default_rng(91).uniform(-1.0, 1.0, pi0.shape))
    other = chain.withParameters(pi1)
    assert np.array_equal(other.getNominalParameters(), pi1) and np.array_equal(chain.getNominalParameters(), pi0)
    assert other.getActiveJointsName() == chain.getActiveJointsName()
    q, dq, ddq = _inputs(n, N, seed=19)
    dev = [_dev(torch, x, "sample") for x in (q, dq, ddq)]
    Y = chain.getRegressor(*dev).cpu().numpy().transpose(0, 2, 1)  # (N, n, P)
    tau = other.getJointTorque(*dev).cpu().numpy()
    err, bound = np.abs(tau - Y @ pi1), 1e-11 * (np.abs(Y) @ np.abs(pi1))
    print("%s: worst |tau' - Y pi'| / |Y| |pi'| %.3g (bound 1e-11)" % (name, (err / bound).max() * 1e-11))
    assert (err <= bound).all() and np.abs(tau - chain.getJointTorque(*dev).cpu().numpy()).max() > 1e-6
