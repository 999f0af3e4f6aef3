"""GPU tests of rdyn_forward_dynamics_vjp_ext / Chain.getJointAccelerationVjp(ext_wrenches=): with ddq = FD_E(q, dq, tau, ext) =
FD_c(q, dq, tau - tau_E(q, ext)), a seed a on ddq and w = M^-1 a
    tau_bar = w,   dq_bar as in getJointAccelerationVjp,   q_bar = -(dtau_dq + diag d tau_c / d q + d tau_E / d q)' w,
    ext_bar = -(d tau_E / d ext)' w.

1. The oracle, residual form (every sample, none excused): the residuals of test_gpu_forward_dynamics_vjp.py with D_E, the derivative of the
   oracle's wrench torque ref.joint_torque(q, 0, 0, ext=W) - ref.joint_torque(q, 0, 0) by the spectral / central-difference scheme of
   test_gpu_torque_derivatives._reference (8-against-16-point gap asserted <= 1e-12 of its scale), added to Dq_ref:
       |q_bar + (Dq_ref + D_E)' tau_bar|_inf <= 1e-11 gscale |tau_bar|_1,   gscale = max(|Dq_ref|_inf, |Dv_ref|_inf) + |tau_ref|_inf + |D_E|_inf + |tau_E|_inf
   and the existing call's q_bar at tau - tau_E violates it on some sample: the wrenches matter.
2. ext_bar, exact linear duality: tau_E = A(q) ext, A built column by column from the library's own getJointTorqueExt(q, 0, 0, unit wrench)
   on the zero-gravity chain; |ext_bar + A' tau_bar| <= 1e-11 (|A|' |tau_bar|) entrywise; the base link's record exactly 0; one-link mode
   equals that link's record of the every-link call to the same bound.
3. The remaining products, subsets, the call without wrenches, a NaN wrench entry, a captured graph."""
import ctypes as C

import numpy as np
import pytest

from _arrays import LAYOUTS, SIZES, _dev, _dev_w, _host, _host_w, _inf, _seed, _state, _wrenches
from _chains import _chain, _trio
from _components import _set, _slopes, _specs
from _references import _WrenchTorque, _bound, _input_types, _reference, _tau_e, _wrench_matrix

pytestmark = pytest.mark.gpu
# planar_2r: the smallest chain; mixed_joints: prismatic joints; ur10_like, panda_like: 6 and 7 joints; ur10_public: fixed head and tail
# links inside a swept chain, the tool a fixed link; ur10_permuted: input order differs from chain order; rev10: the largest register kernel
CHAINS = ["planar_2r", "mixed_joints", "ur10_like", "panda_like", "ur10_public", "ur10_permuted", "rev10"]
EVERY = ("q", "dq", "tau", "ext", "ddq")


def _call(torch, chain, q, dq, tau, a, W, layout, link=None, want=EVERY, **kw):
    """host arrays: status (N,), then the wanted outputs ((N, n); "ext" shaped like W); link: a link index or None"""
    name = None if link is None else chain.getLinksName()[link]
    out = chain.getJointAccelerationVjp(_dev(torch, q, layout), _dev(torch, dq, layout), _dev(torch, tau, layout), _dev(torch, a, layout),
                                        layout=layout, want=want, ext_wrenches=_dev_w(torch, W, layout), ext_link=name, **kw)
    names = (want,) if isinstance(want, str) else want
    return (out[0].cpu().numpy(),) + tuple(_host_w(t, layout, len(q)) if k == "ext" else _host(t, layout) for k, t in zip(names, out[1:]))


def _modes(W, L):
    """(link or None, the wrenches handed over, the same as an every-link array): every link, the tool, a link in the middle"""
    for link in (None, L - 1, L // 2):
        if link is None:
            yield None, W, W
        else:
            Wl = np.zeros_like(W)
            Wl[:, link] = W[:, link]
            yield link, W[:, link], Wl


# ---- 1. the oracle, residual form
@pytest.mark.parametrize("with_components", [False, True], ids=["plain", "components"])
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("name", CHAINS)
def test_against_the_oracle_in_residual_form(name, N, with_components):
    torch = pytest.importorskip("torch")
    chain, ref, chain0 = _trio(name, oracle=True)
    n, L = ref.n, chain.getLinksNumber()
    types = _input_types(chain)
    specs = _specs(n)
    kw = {"components": _set(specs, n)} if with_components else {}
    q, dq, tau = _state(name, n, N, seed=9100 + N)
    a = _seed(n, N, seed=9100 + N)
    W = _wrenches(name, N, L, seed=9200 + N)
    idx = np.arange(n)
    violated = False
    for link, Wgiven, Wl in _modes(W, L):
        DE, _, tauE, gap = _reference(_WrenchTorque(ref, Wl), types, q, dq, np.zeros_like(q))
        escale = _inf(DE) + _inf(tauE)
        # the scale of the construction: the oracle forms tau_E as a DIFFERENCE of two torques that both carry the gravity load, so the
        # rounding of either spectral sum is relative to |tau(q, 0, 0)| too, however small the wrench torque of the sample is
        cscale = escale + _inf(ref.joint_torque(q, np.zeros_like(q), np.zeros_like(q)))
        assert (gap <= 1e-12 * cscale).all(), ("wrench torque, 8 against 16 points", float((gap / cscale).max()))
        cached = None
        for layout in LAYOUTS:
            st, qb, vb, tb, eb, ddq = _call(torch, chain, q, dq, tau, a, Wgiven, layout, link=link, **kw)
            assert st.shape == (N,) and (st == 1).all(), np.unique(st)
            assert all(x.shape == (N, n) and np.isfinite(x).all() for x in (qb, vb, tb, ddq)) and eb.shape == Wgiven.shape
            if cached is None:
                Dq_ref, Dv_ref, tau_ref, gap = _reference(ref, types, q, dq, ddq)
                gscale = np.maximum(_inf(Dq_ref), _inf(Dv_ref)) + _inf(tau_ref)
                assert (gap <= 1e-12 * gscale).all(), ("spectral reference, 8 against 16 points", float((gap / gscale).max()))
                M = ref.joint_inertia(q)
                Dq_all, Dv_all = Dq_ref + DE, Dv_ref.copy()
                if with_components:
                    sq, sv = _slopes(specs, q, dq)
                    Dq_all[:, idx, idx] += sq
                    Dv_all[:, idx, idx] += sv
                cached = (ddq.copy(), M, Dq_all, Dv_all, gscale + escale)
            assert np.array_equal(cached[0], ddq), "the layouts must give the same ddq bits"
            _, M, Dq_all, Dv_all, gscale = cached
            l1 = np.abs(tb).sum(axis=1)
            l1 = np.where(l1 > 0, l1, 1.0)
            mn = np.abs(M).sum(axis=2).max(axis=1)
            r_tau = _inf(np.einsum("sij,sj->si", M, tb) - a) / (mn * _inf(tb) + _inf(a))
            r_q = _inf(qb + np.einsum("sik,si->sk", Dq_all, tb)) / (gscale * l1)
            r_v = _inf(vb + np.einsum("sik,si->sk", Dv_all, tb)) / (gscale * l1)
            print("%s N=%d %s link=%s %s: worst residual ratio tau_bar %.3g q_bar %.3g dq_bar %.3g (bound 1e-11)"
                  % (name, N, "components" if with_components else "plain", link, layout, r_tau.max(), r_q.max(), r_v.max()))
            assert r_tau.max() <= 1e-11 and r_q.max() <= 1e-11 and r_v.max() <= 1e-11, (link, layout, float(r_tau.max()), float(r_q.max()),
                                                                                        float(r_v.max()))
        # the existing call at tau - tau_E lacks d tau_E / d q
        tau_e = _tau_e(torch, chain0, q, Wl)
        old = chain.getJointAccelerationVjp(_dev(torch, q, "sample"), _dev(torch, dq, "sample"), _dev(torch, tau - tau_e, "sample"),
                                            _dev(torch, a, "sample"), want=("q", "tau"), **kw)
        qo, to = old[1].cpu().numpy(), old[2].cpu().numpy()
        lo = np.abs(to).sum(axis=1)
        violated = violated or bool((_inf(qo + np.einsum("sik,si->sk", cached[2], to)) > 1e-11 * cached[4] * np.where(lo > 0, lo, 1.0)).any())
    assert violated, "the wrenches do not matter"


# ---- 2. ext_bar, exact linear duality


@pytest.mark.parametrize("with_components", [False, True], ids=["plain", "components"])
@pytest.mark.parametrize("name", CHAINS)
def test_the_wrench_gradient_is_the_exact_transpose_of_the_wrench_torque(name, with_components):
    torch = pytest.importorskip("torch")
    chain, _, chain0 = _trio(name)
    n, L = chain.getActiveJointsNumber(), chain.getLinksNumber()
    kw = {"components": _set(_specs(n), n)} if with_components else {}
    worst = 0.0
    for N in SIZES:
        q, dq, tau = _state(name, n, N, seed=9300 + N)
        a = _seed(n, N, seed=9300 + N)
        W = _wrenches(name, N, L, seed=9400 + N)
        A = _wrench_matrix(torch, chain0, q, L)
        assert (A[:, :, :6] == 0.0).all() and np.abs(A).max() > 0
        every = None
        for link, Wgiven, _ in _modes(W, L):
            for layout in LAYOUTS:
                st, tb, eb = _call(torch, chain, q, dq, tau, a, Wgiven, layout, link=link, want=("tau", "ext"), **kw)
                assert (st == 1).all() and np.isfinite(eb).all()
                if link is None:
                    assert eb.shape == (N, L, 6) and (eb[:, 0] == 0.0).all() and not np.signbit(eb[:, 0]).any(), "the base link's record is +0.0"
                    want = -np.einsum("sie,si->se", A, tb).reshape(N, L, 6)
                    mag = np.einsum("sie,si->se", np.abs(A), np.abs(tb)).reshape(N, L, 6)
                    if every is None:
                        every = eb
                    assert np.array_equal(every, eb), "the layouts give the same bits"
                else:
                    assert eb.shape == (N, 6)
                    want = -np.einsum("sie,si->se", A[:, :, 6 * link:6 * link + 6], tb)
                    mag = np.einsum("sie,si->se", np.abs(A[:, :, 6 * link:6 * link + 6]), np.abs(tb))
                    assert (np.abs(eb - every[:, link]) <= 1e-11 * mag).all(), (N, link, layout)
                err = np.abs(eb - want)
                assert (err <= 1e-11 * mag).all(), (N, link, layout, float((err / np.where(mag > 0, mag, 1.0)).max()))
                worst = max(worst, float((err[mag > 0] / mag[mag > 0]).max()))
        # the base link alone: the record is +0.0 and the products are the plain ones
        st, qb, eb = _call(torch, chain, q, dq, tau, a, W[:, 0], "sample", link=0, want=("q", "ext"), **kw)
        assert (st == 1).all() and (eb == 0.0).all() and not np.signbit(eb).any()
    print("%s %s: worst |ext_bar + A' tau_bar| / (|A|' |tau_bar|) %.3g (bound 1e-11)" % (name, "components" if with_components else "plain", worst))


# ---- 3. the remaining products
@pytest.mark.parametrize("name", CHAINS)
def test_the_remaining_products_and_subsets(name):
    torch = pytest.importorskip("torch")
    chain, _, chain0 = _trio(name)
    n, L, N = chain.getActiveJointsNumber(), chain.getLinksNumber(), 200
    cs = _set(_specs(n), n)
    q, dq, tau = _state(name, n, N, seed=9500)
    a = _seed(n, N, seed=9500)
    W = _wrenches(name, N, L, seed=9501)
    for link, Wgiven, Wl in _modes(W, L):
        lname = None if link is None else chain.getLinksName()[link]
        tau_e = _tau_e(torch, chain0, q, Wl)
        for kw in ({}, {"components": cs}):
            full = None
            for layout in LAYOUTS:
                got = _call(torch, chain, q, dq, tau, a, Wgiven, layout, link=link, **kw)
                assert (got[0] == 1).all()
                if full is not None:
                    assert all(np.array_equal(x, y) for x, y in zip(full, got)), "the layouts give the same bits"
                full = got
                # ddq: the bits of getJointAcceleration(ext_wrenches=)
                fwd, st = chain.getJointAcceleration(_dev(torch, q, layout), _dev(torch, dq, layout), _dev(torch, tau, layout), layout=layout,
                                                     ext_wrenches=_dev_w(torch, Wgiven, layout), ext_link=lname, **kw)
                assert np.array_equal(_host(fwd, layout), got[5]) and bool((st == 1).all())
            # tau_bar, dq_bar: the existing product at tau - tau_E
            old = chain.getJointAccelerationVjp(_dev(torch, q, "sample"), _dev(torch, dq, "sample"), _dev(torch, tau - tau_e, "sample"),
                                                _dev(torch, a, "sample"), want=("dq", "tau"), **kw)
            bound = _bound(torch, chain, q, dq, tau, tau_e, full[5]) * _inf(a)
            assert (_inf(full[3] - old[2].cpu().numpy()) <= bound).all() and (_inf(full[2] - old[1].cpu().numpy()) <= bound).all()
            # subsets change no bit
            for layout in LAYOUTS:
                for mask in range(1, 32):
                    want = tuple(k for b, k in enumerate(EVERY) if mask >> b & 1)
                    if want == ("ddq",):
                        continue
                    part = _call(torch, chain, q, dq, tau, a, Wgiven, layout, link=link, want=want, **kw)
                    assert np.array_equal(part[0], full[0])
                    for k, t in zip(want, part[1:]):
                        assert np.array_equal(t, full[1 + EVERY.index(k)]), (layout, want, k)
    # tau_bar written over the seed
    ta = _dev(torch, a, "sample")
    out = chain.getJointAccelerationVjp(_dev(torch, q, "sample"), _dev(torch, dq, "sample"), _dev(torch, tau, "sample"), ta, want=EVERY,
                                        ext_wrenches=_dev_w(torch, W, "sample"), components=cs, out={"tau": ta})
    every = _call(torch, chain, q, dq, tau, a, W, "sample", components=cs)
    assert out[3].data_ptr() == ta.data_ptr()
    for k, t, w in zip(EVERY, out[1:], every[1:]):
        assert np.array_equal(t.cpu().numpy(), w), k
    # "ext" needs wrenches; shapes are checked
    tq = _dev(torch, q, "sample")
    with pytest.raises(ValueError):
        chain.getJointAccelerationVjp(tq, tq, tq, tq, want=("q", "ext"))
    with pytest.raises(ValueError, match="Input data dimensions mismatch"):
        chain.getJointAccelerationVjp(tq, tq, tq, tq, ext_wrenches=_dev_w(torch, W[:, 0], "sample"))


def _raw(chain, layout, tq, tdq, ttau, ta, ext, N, outs, stream=None):
    """rdyn_forward_dynamics_vjp_ext itself; outs: (q_bar, dq_bar, tau_bar, ext_bar, ddq, status) tensors or None"""
    import torch
    from rosdyn_amd._lib import Batch, check, lib
    b = Batch()
    b.n_samples, b.q, b.dq, b.ddq = N, tq.data_ptr(), tdq.data_ptr(), None
    b.layout, b.device = (1 if layout == "element" else 0), -1
    b.stream = (stream or torch.cuda.current_stream()).cuda_stream
    px = C.byref(ext) if ext is not None else None
    nbytes = lib().rdyn_forward_dynamics_vjp_ext_workspace_bytes(chain._h, px, 0)
    ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device="cuda")
    p = [t.data_ptr() if t is not None else None for t in outs]
    check(lib().rdyn_forward_dynamics_vjp_ext(chain._h, C.byref(b), None, 0, px, ttau.data_ptr(), ta.data_ptr(), p[0], p[1], p[2], p[3], p[4], p[5],
                                              0, ws.data_ptr(), nbytes))


@pytest.mark.parametrize("name", ["ur10_like", "ur10_public_long", "rev14"])
def test_without_wrenches_the_new_entry_is_the_old_call_bitwise(name):
    torch = pytest.importorskip("torch")
    from rosdyn_amd._lib import ExtWrenches
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 200
    q, dq, tau = _state(name, n, N, seed=9600)
    a = _seed(n, N, seed=9600)
    no_w = ExtWrenches()
    no_w.w, no_w.link, no_w.step_stride = None, 3, 17   # without w nothing else of it is read
    for layout in LAYOUTS:
        tq, tdq, ttau, ta = (_dev(torch, x, layout) for x in (q, dq, tau, a))
        old = chain.getJointAccelerationVjp(tq, tdq, ttau, ta, layout=layout, want=("q", "dq", "tau", "ddq"))
        again = chain.getJointAccelerationVjp(tq, tdq, ttau, ta, layout=layout, want=("q", "dq", "tau", "ddq"), ext_wrenches=None)
        assert all(torch.equal(x, y) for x, y in zip(old, again))
        for ext in (None, no_w):
            outs = [torch.full_like(tq, 777.0) for _ in range(3)] + [None, torch.full_like(tq, 777.0), torch.zeros((N,), dtype=torch.int32, device="cuda")]
            _raw(chain, layout, tq, tdq, ttau, ta, ext, N, outs)
            assert torch.equal(outs[5], old[0])
            for x, y in zip((outs[0], outs[1], outs[2], outs[4]), old[1:]):
                assert torch.equal(x, y)


@pytest.mark.parametrize("name", ["ur10_public", "mixed_joints", "rev10"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_nan_in_one_wrench_entry_fails_that_sample_alone(name, layout):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, L, N = chain.getActiveJointsNumber(), chain.getLinksNumber(), 200
    q, dq, tau = _state(name, n, N, seed=9700)
    a = _seed(n, N, seed=9700)
    W = _wrenches(name, N, L, seed=9701)
    for link in (None, L - 1):
        Wg = W if link is None else W[:, link]
        clean = _call(torch, chain, q, dq, tau, a, Wg, layout, link=link)
        assert (clean[0] == 1).all()
        for bad, value, entry in ((70, np.nan, 2), (3, np.inf, 4), (199, -np.inf, 0)):
            Wb = Wg.copy()
            if link is None:
                Wb[bad, L - 1, entry] = value
            else:
                Wb[bad, entry] = value
            got = _call(torch, chain, q, dq, tau, a, Wb, layout, link=link)
            others = np.arange(N) != bad
            assert got[0][bad] == -1 and (got[0][others] == 1).all()
            for x, y in zip(got[1:], clean[1:]):
                assert np.isnan(x[bad]).all() and np.array_equal(x[others], y[others])
        # a non-finite state or seed fails the sample as in the existing call
        ab = a.copy()
        ab[129, 0] = np.nan
        got = _call(torch, chain, q, dq, tau, ab, Wg, layout, link=link)
        others = np.arange(N) != 129
        assert got[0][129] == -1 and (got[0][others] == 1).all()
        for x, y in zip(got[1:], clean[1:]):
            assert np.isnan(x[129]).all() and np.array_equal(x[others], y[others])
    # the base link's record is not read
    Wb = W.copy()
    Wb[5, 0, :] = np.nan
    got = _call(torch, chain, q, dq, tau, a, Wb, layout)
    clean = _call(torch, chain, q, dq, tau, a, W, layout)
    assert all(np.array_equal(x, y) for x, y in zip(got, clean))


@pytest.mark.parametrize("name", ["ur10_like", "rev10"])
def test_replays_from_a_captured_graph(name):
    """one call captured on a single stream (no side branches), replayed on new inputs"""
    torch = pytest.importorskip("torch")
    from rosdyn_amd._lib import ExtWrenches
    chain = _chain(name)
    n, L, N = chain.getActiveJointsNumber(), chain.getLinksNumber(), 200
    q, dq, tau = _state(name, n, N, seed=9800)
    tq, tdq, ttau = (_dev(torch, x, "sample") for x in (q, dq, tau))
    ta = torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1
    tw = _dev_w(torch, _wrenches(name, N, L, seed=9801), "sample")
    ext = ExtWrenches()
    ext.w, ext.link, ext.step_stride = tw.data_ptr(), -1, 0
    outs = [torch.zeros_like(tq) for _ in range(3)] + [torch.zeros_like(tw), torch.zeros_like(tq), torch.zeros((N,), dtype=torch.int32, device="cuda")]
    _raw(chain, "sample", tq, tdq, ttau, ta, ext, N, outs)   # first use outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            _raw(chain, "sample", tq, tdq, ttau, ta, ext, N, outs, stream=s)
    for k in range(2):
        ta.uniform_(-1, 1)
        tw.uniform_(-1, 1)
        for t in outs:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        again = chain.getJointAccelerationVjp(tq, tdq, ttau, ta, want=EVERY, ext_wrenches=tw)
        assert torch.equal(outs[5], again[0]) and bool((outs[5] == 1).all())
        for x, y in zip(outs[:5], again[1:]):
            assert torch.equal(x, y) and bool(x.abs().sum() > 0)
