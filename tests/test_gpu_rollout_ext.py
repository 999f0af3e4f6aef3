"""GPU tests of the rollouts with external link wrenches, rdyn_rollout_ext / Chain.rollout(ext_wrenches=): T steps over
    ddq = FD_E(q, dq, tau_t, ext_t) = FD_c(q, dq, tau_t - tau_E(q, ext_t)),
the wrench of a step held over the step like the torques and evaluated at every integrator stage at the stage's own q.  Checked against
(a) the library's own getJointAcceleration(ext_wrenches=) at the stage states, one step, (b) the CPU oracle's joint_inertia and
joint_torque(..., ext=) run through the same integrators in numpy, (c) itself: chained calls, per-step sequences, chunk sizes, a captured
graph -- bitwise.  Bounds hold per sample; no sample is excused."""
import ctypes as C

import numpy as np
import pytest

from _arrays import (DT, EPS, INTEGRATORS, LAYOUTS, SIZES, _dev, _dev_seq,
                     _dev_w, _dev_wseq, _host, _inf, _rollout, _wrench_rollout_inputs as _inputs, _wrenches)
from _chains import WRENCH_CHAINS as CHAINS, _trio
from _components import _named_components as _components
from _references import _np_rollout, _oracle_fd_ext

pytestmark = pytest.mark.gpu


def _ext_rollout(torch, chain, q, dq, tau, W, integrator, layout="sample", link=None, seq=False, **kw):
    """W: host wrenches of one step, or with seq a leading T; link: a link index or None"""
    tw = _dev_wseq(torch, W, layout) if seq else _dev_w(torch, W, layout)
    name = None if link is None else chain.getLinksName()[link]
    return _rollout(torch, chain, q, dq, tau, DT, integrator, layout, ext_wrenches=tw, ext_link=name, **kw)


# ---- 5. one step rebuilt from the library's own evaluations
def _lib_fd(torch, chain, W, link):
    """getJointAcceleration(ext_wrenches=) of the library on host arrays -> ddq, the solver term 64 eps cond2(M) max(1, |ddq|) per sample"""
    name = None if link is None else chain.getLinksName()[link]

    def fd(q, dq, tau):
        tq, tdq = _dev(torch, q, "sample"), _dev(torch, dq, "sample")
        a, st = chain.getJointAcceleration(tq, tdq, _dev(torch, tau, "sample"), ext_wrenches=_dev_w(torch, W, "sample"), ext_link=name)
        assert (st.cpu().numpy() == 1).all()
        a = a.cpu().numpy()
        cond = np.linalg.cond(chain.getJointInertia(tq).cpu().numpy())
        return a, 64.0 * EPS * cond * np.maximum(1.0, _inf(a))
    return fd


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_one_step_against_the_library_own_evaluations_with_wrenches(name, integrator):
    """The form and the bounds of test_gpu_rollout.py::test_one_step_against_the_library_own_forward_dynamics, the evaluations being
    getJointAcceleration(ext_wrenches=) at the stage states: a wrench evaluated at the wrong stage state (tau_E depends on q) misses them.
    Every link, and the tool alone."""
    torch = pytest.importorskip("torch")
    chain, _, _ = _trio(name)
    n, L = chain.getActiveJointsNumber(), chain.getLinksNumber()
    worst = 0.0
    for N in SIZES:
        q0, dq0, tau = _inputs(name, n, N, 1, seed=8100 + N)
        W_all = _wrenches(name, N, L, seed=8150 + N)
        for link in (None, L - 1):
            W = W_all if link is None else W_all[:, link]
            fd = _lib_fd(torch, chain, W, link)
            if integrator == "semi_implicit_euler":
                a, solver = fd(q0, dq0, tau[0])
                dq_ref, dq_bound = dq0 + DT * a, DT * solver + 4 * EPS * (_inf(dq0) + DT * _inf(a))
                q_from, q_bound_of = None, lambda dq1: 4 * EPS * (_inf(q0) + DT * _inf(dq1))
            else:
                a1, s1 = fd(q0, dq0, tau[0])
                v2 = dq0 + 0.5 * DT * a1
                a2, s2 = fd(q0 + 0.5 * DT * dq0, v2, tau[0])
                v3 = dq0 + 0.5 * DT * a2
                a3, s3 = fd(q0 + 0.5 * DT * v2, v3, tau[0])
                v4 = dq0 + DT * a3
                a4, s4 = fd(q0 + DT * v3, v4, tau[0])
                dq_ref = dq0 + DT * (a1 / 6 + a2 / 3 + a3 / 3 + a4 / 6)
                dq_bound = DT * (s1 / 6 + s2 / 3 + s3 / 3 + s4 / 6) + 4 * EPS * (_inf(dq0) + DT * (_inf(a1) / 6 + _inf(a2) / 3 + _inf(a3) / 3 + _inf(a4) / 6))
                q_from = q0 + DT * (dq0 / 6 + v2 / 3 + v3 / 3 + v4 / 6)
                q_bound = DT * (0.5 * DT * s1 / 3 + 0.5 * DT * s2 / 3 + DT * s3 / 6) + 4 * EPS * (_inf(q0) + DT * (_inf(dq0) / 6 + _inf(v2) / 3 + _inf(v3) / 3 + _inf(v4) / 6))
            for layout in LAYOUTS:
                q1, dq1, st = _ext_rollout(torch, chain, q0, dq0, tau, W, integrator, layout, link=link)
                assert st.shape == (N,) and (st == 1).all(), np.unique(st)
                edq = _inf(dq1 - dq_ref)
                if q_from is None:
                    eq, qb = _inf(q1 - (q0 + DT * dq1)), q_bound_of(dq1)
                else:
                    eq, qb = _inf(q1 - q_from), q_bound
                worst = max(worst, float((edq / dq_bound).max()), float((eq / qb).max()))
                assert (edq <= dq_bound).all(), (layout, N, link, float((edq / dq_bound).max()), int(np.argmax(edq / dq_bound)))
                assert (eq <= qb).all(), (layout, N, link, float((eq / qb).max()), int(np.argmax(eq / qb)))
            if N == 200:   # the wrenches matter: the rollout without them misses the same bound
                _, dq_plain, _ = _rollout(torch, chain, q0, dq0, tau, DT, integrator)
                assert (_inf(dq_plain - dq_ref) > dq_bound).any()
    print("%s %s: err/bound max %.3g" % (name, integrator, worst))


# ---- 6. multi-step against the oracle
# Measured on the CPU with the oracle alone, on this test's own inputs (T = 8, N = 200, dt = 1e-3, wrenches on every link held over the
# horizon) by the method of test_gpu_rollout.py's MULTI_STEP: the oracle rollout -- joint_inertia and joint_torque(q, dq, 0, ext=W) -- run
# plain and run with every ddq evaluation multiplied by (1 + 1e-11 xi), xi uniform in +-1 per entry.  dev = the largest deviation of the
# end state between the two, relative to max(1, |x|_inf) of the sample's (q, dq); the bound is 8 dev.  max|ddq| = the largest acceleration
# the plain run saw.  Wrench scale: the factor on the wrench entries (uniform in +-1 times the chain's TAU_SCALE) at which the oracle alone
# keeps dev below 1e-9 -- 1 for every chain: nothing had to be shrunk.
WRENCH_SCALE = {name: 1.0 for name in CHAINS}
MULTI_STEP_E = {
    # (chain, integrator): (dev, bound = 8 dev, max|ddq|)
    ("planar_2r", "semi_implicit_euler"): (1.38e-12, 1.1e-11, 70.2),
    ("planar_2r", "rk4"): (1.17e-12, 9.34e-12, 70.2),
    ("ur10_like", "semi_implicit_euler"): (1.64e-11, 1.31e-10, 2.15e+03),
    ("ur10_like", "rk4"): (9.35e-12, 7.48e-11, 2.15e+03),
    ("panda_like", "semi_implicit_euler"): (1.48e-11, 1.18e-10, 1.83e+03),
    ("panda_like", "rk4"): (5.25e-12, 4.2e-11, 1.83e+03),
    ("mixed_joints", "semi_implicit_euler"): (1.42e-11, 1.14e-10, 1.3e+03),
    ("mixed_joints", "rk4"): (6.32e-12, 5.06e-11, 1.3e+03),
    ("ur10_public", "semi_implicit_euler"): (1.15e-11, 9.18e-11, 505),
    ("ur10_public", "rk4"): (3.4e-12, 2.72e-11, 505),
    ("ur10_permuted", "semi_implicit_euler"): (1.3e-11, 1.04e-10, 2.15e+03),
    ("ur10_permuted", "rk4"): (8.26e-12, 6.61e-11, 2.15e+03),
    ("rev10", "semi_implicit_euler"): (9.7e-12, 7.76e-11, 630),
    ("rev10", "rk4"): (4.75e-12, 3.8e-11, 630),
    ("ur10_public_long", "semi_implicit_euler"): (1.47e-11, 1.18e-10, 2.82e+03),
    ("ur10_public_long", "rk4"): (5.04e-12, 4.04e-11, 2.82e+03),
    ("rev14", "semi_implicit_euler"): (8.31e-12, 6.64e-11, 810),
    ("rev14", "rk4"): (4.73e-12, 3.78e-11, 810),
    ("gen20_permuted", "semi_implicit_euler"): (6.15e-12, 4.92e-11, 538),
    ("gen20_permuted", "rk4"): (4.26e-12, 3.41e-11, 538),
}


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_multi_step_against_the_oracle_with_wrenches(name, integrator):
    torch = pytest.importorskip("torch")
    chain, ref, _ = _trio(name, oracle=True)
    N, T = 200, 8
    q0, dq0, tau = _inputs(name, ref.n, N, T, seed=8600)
    W = WRENCH_SCALE[name] * _wrenches(name, N, chain.getLinksNumber(), seed=8601)
    q1, dq1, st = _ext_rollout(torch, chain, q0, dq0, tau, W, integrator)
    assert (st == 1).all()
    qr, dqr = _np_rollout(_oracle_fd_ext(ref, W), q0, dq0, tau, DT, T, integrator)
    scale = np.maximum(1.0, np.maximum(_inf(qr), _inf(dqr)))
    err = np.maximum(_inf(q1 - qr), _inf(dq1 - dqr)) / scale
    bound = MULTI_STEP_E[(name, integrator)][1]
    print("%s %s: err max %.3g (bound %.3g)" % (name, integrator, err.max(), bound))
    assert (err <= bound).all(), (float(err.max()), bound, int(np.argmax(err)))


# ---- 7. a per-step wrench sequence; the horizon can be split, bitwise
@pytest.mark.parametrize("name", ["ur10_like", "mixed_joints", "rev10", "ur10_public_long", "rev14"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_a_wrench_sequence_is_the_chained_one_step_calls_and_the_horizon_splits_bitwise(name, integrator):
    torch = pytest.importorskip("torch")
    chain, _, _ = _trio(name)
    n, L, N, T = chain.getActiveJointsNumber(), chain.getLinksNumber(), 200, 7
    q0, dq0, tau = _inputs(name, n, N, T, seed=8700)
    W_all = np.stack([_wrenches(name, N, L, seed=8710 + t) for t in range(T)])
    for link in (None, L - 1):
        W = W_all if link is None else W_all[:, :, link]
        whole = _ext_rollout(torch, chain, q0, dq0, tau, W, integrator, link=link, seq=True)
        assert (whole[2] == 1).all() and np.isfinite(whole[0]).all() and np.isfinite(whole[1]).all()
        # T chained one-step calls, each with its step's wrench held constant
        q, dq = q0, dq0
        for t in range(T):
            q, dq, st = _ext_rollout(torch, chain, q, dq, tau[t:t + 1], W[t], integrator, link=link)
            assert (st == 1).all()
        assert np.array_equal(q, whole[0]) and np.array_equal(dq, whole[1]), link
        # split at t = 3: the later call starts at its own step's record
        q, dq, _ = _ext_rollout(torch, chain, q0, dq0, tau[:3], W[:3], integrator, link=link, seq=True)
        q, dq, _ = _ext_rollout(torch, chain, q, dq, tau[3:], W[3:], integrator, link=link, seq=True)
        assert np.array_equal(q, whole[0]) and np.array_equal(dq, whole[1]), link
        # element-major equals sample-major; a sequence of equal records equals the constant wrench
        el = _ext_rollout(torch, chain, q0, dq0, tau, W, integrator, "element", link=link, seq=True)
        assert all(np.array_equal(a, b) for a, b in zip(el, whole))
        const = _ext_rollout(torch, chain, q0, dq0, tau, W[0], integrator, link=link)
        same = _ext_rollout(torch, chain, q0, dq0, tau, np.stack([W[0]] * T), integrator, link=link, seq=True)
        assert all(np.array_equal(a, b) for a, b in zip(const, same))
        assert not np.array_equal(const[0], whole[0])
    with pytest.raises(ValueError, match="Input data dimensions mismatch"):   # fewer records than steps
        _ext_rollout(torch, chain, q0, dq0, tau, W_all[:T - 1], integrator, seq=True)


# ---- 8. trajectory records, aliasing, sticky status
@pytest.mark.parametrize("name", ["ur10_like", "rev14"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_trajectory_records_aliasing_and_sticky_status_with_wrenches(name, integrator):
    torch = pytest.importorskip("torch")
    chain, _, _ = _trio(name)
    n, L, N, T = chain.getActiveJointsNumber(), chain.getLinksNumber(), 200, 5
    q0, dq0, tau = _inputs(name, n, N, T, seed=8800)
    W = np.stack([_wrenches(name, N, L, seed=8810 + t) for t in range(T)])
    ends = [_ext_rollout(torch, chain, q0, dq0, tau, W, integrator, n_steps=k, seq=True) for k in range(1, T + 1)]
    for layout in LAYOUTS:
        # trajectory_every = 2: two records, the states after steps 2 and 4
        q1, dq1, st, qt, dqt = _ext_rollout(torch, chain, q0, dq0, tau, W, integrator, layout, seq=True, trajectory_every=2)
        assert (st == 1).all() and qt.shape == (2, N, n)
        assert np.array_equal(q1, ends[T - 1][0]) and np.array_equal(dq1, ends[T - 1][1])
        for k in range(2):
            assert np.array_equal(qt[k], ends[2 * k + 1][0]) and np.array_equal(dqt[k], ends[2 * k + 1][1]), (layout, k)
        # q_end aliasing q0, dq_end aliasing dq0
        tq, tdq = _dev(torch, q0, layout), _dev(torch, dq0, layout)
        r = chain.rollout(tq, tdq, _dev_seq(torch, tau, layout), DT, integrator=integrator, layout=layout, out=(tq, tdq),
                          ext_wrenches=_dev_wseq(torch, W, layout))
        assert r[0] is tq and np.array_equal(_host(tq, layout), ends[T - 1][0]) and np.array_equal(_host(tdq, layout), ends[T - 1][1])
        # one sample that cannot be solved (a NaN coordinate: its M is NaN and fails the pivot rule at the first evaluation): status -1 and
        # NaN on that sample from the first record on, every other sample bitwise what it was
        bad = 37
        qb = q0.copy()
        qb[bad, 0] = np.nan
        q1, dq1, st, qt, dqt = _ext_rollout(torch, chain, qb, dq0, tau, W, integrator, layout, seq=True, trajectory_every=1)
        others = np.arange(N) != bad
        assert st[bad] == -1 and (st[others] == 1).all()
        assert np.isnan(q1[bad]).all() and np.isnan(dq1[bad]).all() and np.isnan(qt[:, bad]).all() and np.isnan(dqt[:, bad]).all()
        assert np.array_equal(q1[others], ends[T - 1][0][others]) and np.array_equal(dq1[others], ends[T - 1][1][others])
        for k in range(T):
            assert np.array_equal(qt[k][others], ends[k][0][others])
    # a non-finite wrench entry: NaN by propagation on that sample alone; one evaluation keeps status 1 (the pivot rule looks at M, which
    # the wrenches do not enter), a rollout reports -1 from the next evaluation on (include/rdyn.h)
    Wn = W.copy()
    Wn[0, bad, L - 1, 2] = np.nan
    q1, dq1, st = _ext_rollout(torch, chain, q0, dq0, tau, Wn, integrator, seq=True)
    assert st[bad] == -1 and (st[others] == 1).all() and np.isnan(q1[bad]).all()
    assert np.array_equal(q1[others], ends[T - 1][0][others])
    ddq, st = chain.getJointAcceleration(_dev(torch, q0, "sample"), _dev(torch, dq0, "sample"), _dev(torch, tau[0], "sample"),
                                         ext_wrenches=_dev_w(torch, Wn[0], "sample"))
    assert bool((st == 1).all()) and bool(torch.isnan(ddq[bad]).all()) and bool(torch.isfinite(ddq[others]).all())


# ---- 9. the chunk size does not change the result
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_chunk_size_does_not_change_the_result_with_wrenches(integrator):
    """rev14, chunk_samples 0 and 16384 + 64.  The library applies a floor of 16 384 samples per chunk only to its DEFAULT (include/rdyn.h:
    chunk_samples = 0); N = 16384 + 65 is the smallest batch that 16384 + 64 splits into more than one chunk -- a full one and a single
    sample -- and the workspace query shows that it does."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd._lib import ExtWrenches, RolloutDesc, lib
    chain, _, _ = _trio("rev14")
    n, L, T, chunk = 14, chain.getLinksNumber(), 2, 16384 + 64
    N = chunk + 1
    x, d = ExtWrenches(), RolloutDesc()
    x.w, x.link = 4096, -1
    d.integrator = 1 if integrator == "rk4" else 0
    need = lambda c: lib().rdyn_rollout_ext_workspace_bytes(chain._h, C.byref(d), C.byref(x), N, c)
    assert need(chunk) < need(N)   # more than one chunk: the image of a chunk is smaller than the image of the whole batch
    q0, dq0, tau = _inputs("rev14", n, N, T, seed=8900)
    W = np.stack([_wrenches("rev14", N, L, seed=8910 + t) for t in range(T)])
    a = _ext_rollout(torch, chain, q0, dq0, tau, W, integrator, seq=True, trajectory_every=1, chunk_samples=0)
    b = _ext_rollout(torch, chain, q0, dq0, tau, W, integrator, seq=True, trajectory_every=1, chunk_samples=chunk)
    assert (a[2] == 1).all()
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    c = _ext_rollout(torch, chain, q0, dq0, tau, W[:, :, L - 1], integrator, "element", link=L - 1, seq=True, chunk_samples=0)
    e = _ext_rollout(torch, chain, q0, dq0, tau, W[:, :, L - 1], integrator, "element", link=L - 1, seq=True, chunk_samples=chunk)
    assert all(np.array_equal(u, v) for u, v in zip(c, e)) and not np.array_equal(c[0], a[0])


# ---- 4'. without wrenches the new entry is the old call, bitwise (T = 5)
@pytest.mark.parametrize("name", ["ur10_like", "rev14"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_without_wrenches_the_new_entry_is_the_old_rollout_bitwise(name, integrator):
    torch = pytest.importorskip("torch")
    from rosdyn_amd._lib import INTEGRATORS as CODES, Batch, ExtWrenches, RolloutDesc, check, lib
    chain, _, _ = _trio(name)
    n, N, T = chain.getActiveJointsNumber(), 200, 5
    q0, dq0, tau = _inputs(name, n, N, T, seed=9000)
    cs = _components(name, n)
    no_w = ExtWrenches()
    no_w.w, no_w.link, no_w.step_stride = None, 99, -4   # without w nothing else of it is read
    tq, tdq, ttau = _dev(torch, q0, "sample"), _dev(torch, dq0, "sample"), torch.from_numpy(tau).cuda()
    for comps in (None, cs):
        old = chain.rollout(tq, tdq, ttau, DT, integrator=integrator, components=comps)
        for ext in (None, no_w):
            b = Batch()
            b.n_samples, b.q, b.dq, b.ddq, b.layout, b.device = N, tq.data_ptr(), tdq.data_ptr(), None, 0, -1
            b.stream = torch.cuda.current_stream().cuda_stream
            q1, dq1 = torch.full_like(tq, 777.0), torch.full_like(tq, 777.0)
            st = torch.zeros((N,), dtype=torch.int32, device="cuda")
            d = RolloutDesc()
            d.n_steps, d.integrator, d.dt, d.tau, d.tau_step_stride = T, CODES[integrator], DT, ttau.data_ptr(), n * N
            d.q_end, d.dq_end, d.status = q1.data_ptr(), dq1.data_ptr(), st.data_ptr()
            px = C.byref(ext) if ext is not None else None
            nbytes = lib().rdyn_rollout_ext_workspace_bytes(chain._h, C.byref(d), px, N, 0)
            assert nbytes == lib().rdyn_rollout_workspace_bytes(chain._h, C.byref(d), N, 0)
            ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device="cuda")
            cp, k = chain._component_list(comps) if comps is not None else (None, 0)
            check(lib().rdyn_rollout_ext(chain._h, C.byref(b), C.byref(d), cp, k, px, 0, ws.data_ptr(), nbytes))
            assert torch.equal(q1, old[0]) and torch.equal(dq1, old[1]) and torch.equal(st, old[2])


# ---- 10. graph capture
def test_a_rollout_with_wrenches_replays_from_a_captured_graph():
    """tests/test_gpu_graph.py's pattern: first use outside capture, one capture on a single side stream, replays on fresh inputs in the
    captured buffers give the bits of the eager call."""
    torch = pytest.importorskip("torch")
    chain, _, _ = _trio("ur10_like")
    n, L, N, T = chain.getActiveJointsNumber(), chain.getLinksNumber(), 5000, 4
    q, dq = (torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(2))
    tau = torch.rand((T, N, n), dtype=torch.float64, device="cuda") * 0.8 - 0.4
    W = torch.rand((T, N, L, 6), dtype=torch.float64, device="cuda") * 0.8 - 0.4
    q_end, dq_end = torch.empty_like(q), torch.empty_like(q)
    chain.rollout(q, dq, tau, DT, integrator="rk4", out=(q_end, dq_end), ext_wrenches=W)   # first use outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            _, _, st = chain.rollout(q, dq, tau, DT, integrator="rk4", out=(q_end, dq_end), ext_wrenches=W)
    for k in range(2):
        q.uniform_(-1, 1)
        dq.uniform_(-1, 1)
        tau.uniform_(-0.4, 0.4)
        W.uniform_(-0.4, 0.4)
        q_end.zero_()
        dq_end.zero_()
        st.zero_()
        g.replay()
        torch.cuda.synchronize()
        q2, dq2, st2 = chain.rollout(q, dq, tau, DT, integrator="rk4", ext_wrenches=W)
        assert torch.equal(q_end, q2) and torch.equal(dq_end, dq2) and torch.equal(st, st2) and bool((st == 1).all())
