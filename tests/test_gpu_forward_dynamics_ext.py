"""GPU tests of the forward dynamics with external link wrenches, rdyn_forward_dynamics_ext / Chain.getJointAcceleration(ext_wrenches=):
    FD_E(q, dq, tau, ext) = FD_c(q, dq, tau - tau_E(q, ext)),
tau_E the joint torque of the wrenches alone in the convention of getJointTorque(q, Dq, DDq, ext_wrenches_in_link_frame).

Yardsticks (each bound holds per sample, no sample is excused):
  the composition         getJointAcceleration(q, dq, tau - tau_E) with tau_E from the library's own getJointTorqueExt(q, 0, 0, W) on a
                          ZERO-GRAVITY Chain of the same URDF (no gravity torque to cancel):
                          |ddq_E - ddq_comp|_inf <= 64 eps (cond2(M) max(1, |ddq|_inf) + |M^-1|_2 (|tau|_2 + |h|_2 + |tau_E|_2));
                          the first term is the project's solver bound (test_gpu_forward_dynamics.py), the second covers the different
                          rounding of the right-hand side (the wrench enters the link wrenches, not the torque vector).
  the reference           |M_ref ddq + ref.joint_torque(q, dq, 0, ext=W) - tau|_inf <= 1e-11 (|M_ref|_inf |ddq|_inf + |tau|_inf + |h|_inf
                          + |tau_E|_inf): the residual test of test_gpu_forward_dynamics.py with the wrench torque in the scale.  This pins the
                          reference's wrench convention, twist-form transform included."""
import ctypes as C

import numpy as np
import pytest

from _arrays import LAYOUTS, SIZES, _dev, _dev_w, _inf, _solve, _state, _wrenches
from _chains import WRENCH_CHAINS as CHAINS, _chain, _trio
from _components import _named_components as _components
from _references import _bound, _tau_e

pytestmark = pytest.mark.gpu


def _ext_solve(torch, chain, q, dq, tau, W, layout, link=None, **kw):
    return _solve(torch, chain, q, dq, tau, layout, ext_wrenches=_dev_w(torch, W, layout), ext_link=link, **kw)


# ---- 1. one evaluation against the composition
@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("with_components", [False, True])
def test_one_evaluation_against_the_composition(name, with_components):
    """Every link and one link (the tool, a link in the middle), with and without a ComponentSet, every size and both layouts; and the plain
    call without wrenches violates the bound on some sample: the wrenches matter."""
    torch = pytest.importorskip("torch")
    chain, _, chain0 = _trio(name)
    n, L, links = chain.getActiveJointsNumber(), chain.getLinksNumber(), chain.getLinksName()
    kw = {"components": _components(name, n)} if with_components else {}
    worst = 0.0
    for N in SIZES:
        q, dq, tau = _state(name, n, N, seed=7100 + N)
        W = _wrenches(name, N, L, seed=7200 + N)
        for link in (None, L - 1, L // 2):
            Wl = W
            if link is not None:
                Wl = np.zeros_like(W)
                Wl[:, link] = W[:, link]
            tau_e = _tau_e(torch, chain0, q, Wl)
            comp, st = _solve(torch, chain, q, dq, tau - tau_e, "sample", **kw)
            assert (st == 1).all()
            bound = _bound(torch, chain, q, dq, tau, tau_e, comp)
            for layout in LAYOUTS:
                got, st = _ext_solve(torch, chain, q, dq, tau, Wl if link is None else W[:, link], layout,
                                     link=None if link is None else links[link], **kw)
                assert st.shape == (N,) and (st == 1).all(), np.unique(st)
                ratio = _inf(got - comp) / bound
                worst = max(worst, float(ratio.max()))
                assert (ratio <= 1.0).all(), (N, link, layout, float(ratio.max()), int(np.argmax(ratio)))
            if N == 200:
                plain, _ = _solve(torch, chain, q, dq, tau, "sample", **kw)
                assert (_inf(plain - comp) > bound).any(), (link, "the wrenches do not matter")
    print("%s components=%s: max err/bound %.3g" % (name, with_components, worst))


# ---- 2. one evaluation against the reference restatement
@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_evaluation_against_the_reference_restatement(name, layout):
    torch = pytest.importorskip("torch")
    chain, ref, _ = _trio(name, oracle=True)
    n, L, N = ref.n, chain.getLinksNumber(), 200
    q, dq, tau = _state(name, n, N, seed=7300)
    W = _wrenches(name, N, L, seed=7301)
    ddq, st = _ext_solve(torch, chain, q, dq, tau, W, layout)
    assert (st == 1).all() and np.isfinite(ddq).all()
    M = ref.joint_inertia(q)
    zero = np.zeros_like(q)
    h = ref.joint_torque(q, dq, zero)
    h_ext = ref.joint_torque(q, dq, zero, ext=W)
    tau_e = h_ext - h
    res = _inf(np.einsum("sij,sj->si", M, ddq) + h_ext - tau)
    scale = np.abs(M).sum(axis=2).max(axis=1) * _inf(ddq) + _inf(tau) + _inf(h) + _inf(tau_e)
    print("%s %s: residual ratio max %.3g (bound 1e-11), |tau_E| / |tau| median %.3g" % (name, layout, (res / scale).max(),
                                                                                          np.median(_inf(tau_e) / _inf(tau))))
    assert (res <= 1e-11 * scale).all(), (float((res / scale).max()), int(np.argmax(res / scale)))
    # ... and the wrenches are seen: without them the residual of the same ddq is the wrench torque
    assert (_inf(np.einsum("sij,sj->si", M, ddq) + h - tau) > 1e-11 * scale).any()


# ---- 3. one link equals every link with the other records zero; the base link changes nothing
@pytest.mark.parametrize("name", CHAINS)
def test_single_link_mode_equals_all_link_mode_and_the_base_link_changes_nothing(name):
    torch = pytest.importorskip("torch")
    chain, _, chain0 = _trio(name)
    n, L, links, N = chain.getActiveJointsNumber(), chain.getLinksNumber(), chain.getLinksName(), 200
    q, dq, tau = _state(name, n, N, seed=7400)
    W = _wrenches(name, N, L, seed=7401)
    for link in range(L):
        Wl = np.zeros_like(W)
        Wl[:, link] = W[:, link]
        tau_e = _tau_e(torch, chain0, q, Wl) if link else np.zeros_like(q)
        every, st = _ext_solve(torch, chain, q, dq, tau, Wl, "sample")
        assert (st == 1).all()
        bound = _bound(torch, chain, q, dq, tau, tau_e, every)
        for layout in LAYOUTS:
            one, st = _ext_solve(torch, chain, q, dq, tau, W[:, link], layout, link=links[link])
            assert (st == 1).all()
            assert (_inf(one - every) <= bound).all(), (link, layout, float((_inf(one - every) / bound).max()))
        if link == 0:
            plain, _ = _solve(torch, chain, q, dq, tau, "sample")
            assert (_inf(every - plain) <= bound).all() and (_inf(one - plain) <= bound).all()
    with pytest.raises(ValueError):
        _ext_solve(torch, chain, q, dq, tau, W[:, 0], "sample", link="no_such_link")
    for bad in (W[:, :-1], W[:-1], W[:, 0]):   # a link short, a sample short, one link's record without ext_link
        if bad.size:
            with pytest.raises(ValueError, match="Input data dimensions mismatch"):
                _ext_solve(torch, chain, q, dq, tau, bad, "sample")


# ---- 4. without wrenches the new entry is the old call, bitwise
def _raw_fd(chain, layout, tq, tdq, ttau, ext, N, comps=None):
    import torch
    from rosdyn_amd._lib import Batch, check, lib
    b = Batch()
    b.n_samples, b.q, b.dq, b.ddq = N, tq.data_ptr(), tdq.data_ptr(), None
    b.layout, b.device, b.stream = (1 if layout == "element" else 0), -1, torch.cuda.current_stream().cuda_stream
    px = C.byref(ext) if ext is not None else None
    nbytes = lib().rdyn_forward_dynamics_ext_workspace_bytes(chain._h, px, 0)
    assert nbytes == lib().rdyn_forward_dynamics_workspace_bytes(chain._h, 0)
    ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device="cuda")
    ddq = torch.full_like(tq, 777.0)
    st = torch.zeros((N,), dtype=torch.int32, device="cuda")
    cp, k = chain._component_list(comps) if comps is not None else (None, 0)
    check(lib().rdyn_forward_dynamics_ext(chain._h, C.byref(b), cp, k, px, ttau.data_ptr(), ddq.data_ptr(), st.data_ptr(), 0, ws.data_ptr(), nbytes))
    return ddq, st


@pytest.mark.parametrize("name", ["ur10_like", "rev14"])
def test_without_wrenches_the_new_entry_is_the_old_call_bitwise(name):
    torch = pytest.importorskip("torch")
    from rosdyn_amd._lib import ExtWrenches
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 200
    q, dq, tau = _state(name, n, N, seed=7500)
    cs = _components(name, n)
    no_w = ExtWrenches()
    no_w.w, no_w.link, no_w.step_stride = None, 3, 17   # without w nothing else of it is read
    for layout in LAYOUTS:
        tq, tdq, ttau = _dev(torch, q, layout), _dev(torch, dq, layout), _dev(torch, tau, layout)
        for comps in (None, cs):
            old, old_st = chain.getJointAcceleration(tq, tdq, ttau, layout=layout, components=comps)
            for ext in (None, no_w):
                new, new_st = _raw_fd(chain, layout, tq, tdq, ttau, ext, N, comps)
                assert torch.equal(new, old) and torch.equal(new_st, old_st)
