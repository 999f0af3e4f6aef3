"""GPU tests of rdyn_rollout_adjoint / Chain.rolloutAdjoint: the exact transpose of the discrete scheme Chain.rollout integrates.

1. One step against the library's own product (Chain.getJointAccelerationVjp), composed in numpy by the step transposes of include/rdyn.h;
   the RK4 stage states rebuilt in numpy from getJointAcceleration.  Bound per sample and entry: 1e-11 x the sum of the absolute terms of
   the entry (the same composition run on magnitudes: |lambda|, and |matrix| |seed| for every product, the matrices from
   getJointAccelerationDerivatives).  Only stage-state roundings and fma contraction separate the two sides; the worst ratio is printed.
2. A horizon split anywhere into two chained calls gives the single call's bits (running seeds on every record, gtau per step).
   Together with 1 this pins every multi-step result to a chain of verified single steps.
3. Directional consistency against central differences of Chain.rollout itself (not a parity bound), see the table at the test.
4. Failures, zero seeds, T = 0, the summed torque gradient, aliasing, the chunk size, a captured graph."""
import ctypes as C

import numpy as np
import pytest

from _arrays import EPS, INTEGRATORS, _adjoint, _adjoint_inputs as _inputs, _dev, _dev_seq, _directional_inputs, _forward, _host, _host_seq, _seeds
from _chains import _chain, _pair
from _components import _set, _specs
from _references import _input_types, _lib_abs_vjp, _lib_fd, _lib_vjp, _np_adjoint, _np_rollout, _np_step, _np_step_adjoint, _oracle_fd, _reference

pytestmark = pytest.mark.gpu
SWEPT = ["planar_2r", "ur10_like", "panda_like", "mixed_joints", "ur10_public_long", "rev10"]
LONG = ["rev14", "gen20_permuted"]


# ---- the step transposes in numpy over any product vjp(q, v, tau, seed) -> (q_bar, v_bar, tau_bar) and forward dynamics fd(q, v, tau) -> ddq


# ---- 1. one step against the library's own product
@pytest.mark.parametrize("with_components", [False, True], ids=["plain", "components"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", SWEPT + LONG)
def test_one_step_against_the_library_own_product(name, integrator, with_components):
    """Expected distance: a few eps of the magnitudes (the kernel contracts lv + dt lq and the stage updates into fmas, numpy rounds twice;
    the seed handed to the product then differs in its last bit).  The worst ratio distance / magnitude is printed; the bound is 1e-11."""
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, dt = chain.getActiveJointsNumber(), 1e-3
    cs = _set(_specs(n), n) if with_components else None
    fd, vjp, avjp = _lib_fd(torch, chain, cs), _lib_vjp(torch, chain, cs), _lib_abs_vjp(torch, chain, cs)
    worst = 0.0
    for N in (1, 63, 64, 65, 200):
        q0, dq0, tau = _inputs(name, n, N, 1, seed=6100 + N)
        gq, gv, _, _ = _seeds(n, N, 1, seed=6100 + N)
        want = _np_step_adjoint(vjp, fd, q0, dq0, tau[0], gq, gv, dt, integrator)
        mag = _np_step_adjoint(avjp, fd, q0, dq0, tau[0], np.abs(gq), np.abs(gv), dt, integrator)
        got = None
        for layout in ("sample", "element"):
            fw = (_dev(torch, q0, layout), _dev(torch, dq0, layout), _dev_seq(torch, tau, layout), None, None)
            r = _adjoint(torch, chain, fw, dt, integrator, layout, gq_end=gq, gdq_end=gv, components=cs)
            assert r[3].shape == (N,) and (r[3] == 1).all(), np.unique(r[3])
            if got is not None:
                assert all(np.array_equal(x, y) for x, y in zip(got, r)), "the layouts give the same bits"
            got = r
        for what, g, w, m in zip(("gq0", "gdq0", "gtau"), (got[0], got[1], got[2][0]), want, mag):
            assert np.isfinite(g).all() and (m > 0).all()
            ratio = float((np.abs(g - w) / m).max())
            worst = max(worst, ratio)
            assert ratio <= 1e-11, (what, N, ratio)
    print("%s %s %s: worst distance / sum of absolute terms %.3g (bound 1e-11)" % (name, integrator, "components" if with_components else "plain", worst))


# ---- 2. the horizon can be split anywhere, bitwise
@pytest.mark.parametrize("layout", ["sample", "element"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", SWEPT + LONG)
def test_the_horizon_can_be_split_anywhere_bitwise(name, integrator, layout):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N, T, dt = chain.getActiveJointsNumber(), 65, 6, 1e-3
    cs = _set(_specs(n), n)
    q0, dq0, tau = _inputs(name, n, N, T, seed=6400)
    gq, gv, rq, rv = _seeds(n, N, T, seed=6400)
    fw, st = _forward(torch, chain, q0, dq0, tau, dt, integrator, layout, components=cs)
    assert (st == 1).all()
    tq, tdq, ttau, q_traj, dq_traj = fw
    whole = _adjoint(torch, chain, fw, dt, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, components=cs)
    assert (whole[3] == 1).all() and all(np.isfinite(x).all() for x in whole[:3])
    assert whole[2].shape == (T, N, n) and not np.array_equal(whole[0], gq)
    for cut in ((3,) if name in LONG else range(1, T)):
        # the later part: steps cut .. T - 1 from x_cut = record cut - 1, the running seeds of its own records
        later = (q_traj[cut - 1], dq_traj[cut - 1], ttau[cut:], q_traj[cut:], dq_traj[cut:])
        b = _adjoint(torch, chain, later, dt, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq[cut:], gdq_traj=rv[cut:], components=cs)
        # the earlier part: its end seeds are the later part's result
        earlier = (tq, tdq, ttau[:cut], q_traj[:cut], dq_traj[:cut])
        a = _adjoint(torch, chain, earlier, dt, integrator, layout, gq_end=b[0], gdq_end=b[1], gq_traj=rq[:cut], gdq_traj=rv[:cut], components=cs)
        assert np.array_equal(a[0], whole[0]) and np.array_equal(a[1], whole[1]), cut
        assert np.array_equal(np.concatenate([a[2], b[2]]), whole[2]), cut
        assert (a[3] == 1).all() and (b[3] == 1).all()


# ---- 3. directional consistency
# L = <c_q, q_T> + <c_v, dq_T>, T = 8, dt = 1e-2, N = 200; the gradient of the adjoint call along (e, f) on (q0, dq0) -- entries uniform in
# +-1, h = 2^-9 and 2^-10 -- and along g on tau -- entries uniform in +-TAU_SCALE, h = 2^-7 and 2^-8 -- against the central difference of
# Chain.rollout itself.  err = |difference| / scale per sample, scale = the largest |term| of the sample's inner product.  The rollout is
# smooth, so the error of the central difference is h^2 / 6 |L'''| + O(h^4): err(h) / err(h / 2) = 4.
# Measured on the CPU ORACLE alone with this test's own inputs (_directional_inputs; _measure_directional_on_the_oracle below): a numpy rollout of the oracle's forward dynamics
# (test_gpu_rollout.py: _np_rollout over _oracle_fd) against the numpy adjoint above (_np_adjoint) with the oracle's exact matrices
# (-M_ref^-1 D_ref, D_ref the spectral derivative of test_gpu_torque_derivatives.py).  err at the larger h, worst over the samples, Euler /
# RK4; ratio = err at the larger h over err at the smaller, range over both integrators on the samples with err >= 1e-9:
#     chain         direction   err / scale, worst (Euler / RK4)   ratio              samples >= 1e-9 scale (Euler / RK4)
#     planar_2r     x0          1.41e-5 / 1.47e-5                  [3.9941, 4.0091]   199 / 199 of 200
#     planar_2r     tau         5.28e-7 / 6.07e-7                  [3.9740, 4.0174]   125 / 124 of 200
#     ur10_like     x0          2.01e-5 / 2.03e-5                  [3.9925, 4.0048]   200 / 200 of 200
#     ur10_like     tau         1.28e-6 / 1.45e-6                  [3.9953, 4.0060]   167 / 164 of 200
#     panda_like    x0          2.91e-4 / 3.50e-4                  [3.9919, 4.0294]   200 / 200 of 200
#     panda_like    tau         8.44e-6 / 1.00e-5                  [3.9988, 4.0008]   198 / 198 of 200
#     mixed_joints  x0          9.65e-5 / 1.02e-4                  [3.9941, 4.0028]   200 / 200 of 200
#     mixed_joints  tau         3.47e-6 / 3.94e-6                  [3.9956, 4.0054]   181 / 179 of 200
#     rev10         x0          1.66e-4 / 1.86e-4                  [3.9985, 4.0010]   200 / 200 of 200
#     rev10         tau         1.41e-5 / 1.44e-5                  [3.9986, 4.0058]   200 / 199 of 200
#     rev14         x0          3.66e-5 / 3.68e-5                  [3.9985, 4.0034]   200 / 200 of 200
#     rev14         tau         3.09e-5 / 3.85e-5                  [3.9940, 4.0133]   200 / 200 of 200
# The oracle alone meets both conditions on every chain with these settings (ratio in [3.5, 4.5] on at least half of the batch).
DIRECTIONAL = {
    # chain: ((x0 err Euler, RK4), (tau err Euler, RK4)): the table's worst figures
    "planar_2r": ((1.41e-5, 1.47e-5), (5.28e-7, 6.07e-7)),
    "ur10_like": ((2.01e-5, 2.03e-5), (1.28e-6, 1.45e-6)),
    "panda_like": ((2.91e-4, 3.50e-4), (8.44e-6, 1.00e-5)),
    "mixed_joints": ((9.65e-5, 1.02e-4), (3.47e-6, 3.94e-6)),
    "rev10": ((1.66e-4, 1.86e-4), (1.41e-5, 1.44e-5)),
    "rev14": ((3.66e-5, 3.68e-5), (3.09e-5, 3.85e-5)),
}
DIRECTIONAL_CHAINS = ["planar_2r", "ur10_like", "panda_like", "mixed_joints", "rev10", "rev14"]


def _directional_errors(loss, grads, q0, dq0, tau, e, f, g):
    """loss(q0, dq0, tau) -> (N,); grads = (gq0, gdq0, gtau).  Returns {direction: (err at the larger h, err at the smaller h)} per sample"""
    gq0, gdq0, gtau = grads
    out = {}
    tx = np.concatenate([gq0 * e, gdq0 * f], axis=1)
    tt = np.moveaxis(gtau * g, 0, 1).reshape(len(q0), -1)
    for what, terms, hs, move in (("x0", tx, (2.0 ** -9, 2.0 ** -10), lambda h: (q0 + h * e, dq0 + h * f, tau)),
                                  ("tau", tt, (2.0 ** -7, 2.0 ** -8), lambda h: (q0, dq0, tau + h * g))):
        lin, scale = terms.sum(axis=1), np.abs(terms).max(axis=1)
        out[what] = tuple(np.abs((loss(*move(h)) - loss(*move(-h))) / (2.0 * h) - lin) / scale for h in hs)
    return out


def _measure_directional_on_the_oracle(names=DIRECTIONAL_CHAINS):
    """the table above: `python tests/test_gpu_rollout_adjoint.py [chain ...]` on the CPU (no GPU, no library call besides building the chain)"""
    N, T, dt = 200, 8, 1e-2
    for name in names:
        chain, ref = _pair(name)
        types = _input_types(chain)
        q0, dq0, tau, cq, cv, e, f, g = _directional_inputs(name, ref.n, N, T)
        fd = _oracle_fd(ref)

        def vjp(q, v, u, seed):
            M = ref.joint_inertia(q)
            a = np.linalg.solve(M, (u - ref.joint_torque(q, v, np.zeros_like(q)))[:, :, None])[:, :, 0]
            w = np.linalg.solve(M, seed[:, :, None])[:, :, 0]
            Dq, Dv, _, _ = _reference(ref, types, q, v, a)
            return -np.einsum("sik,si->sk", Dq, w), -np.einsum("sik,si->sk", Dv, w), w

        for integrator in INTEGRATORS:
            q, v, qs, vs = q0, dq0, [], []
            for t in range(T):
                q, v = _np_step(fd, q, v, tau[t], dt, integrator)
                qs.append(q)
                vs.append(v)
            grads = _np_adjoint(vjp, fd, q0, dq0, tau, np.array(qs), np.array(vs), cq, cv, dt, integrator)

            def loss(a, b, u):
                qe, ve = _np_rollout(fd, a, b, u, dt, T, integrator)
                return (cq * qe).sum(axis=1) + (cv * ve).sum(axis=1)

            for what, (big, small) in _directional_errors(loss, grads, q0, dq0, tau, e, f, g).items():
                sel = big >= 1e-9
                ratio = big[sel] / small[sel]
                print("%-14s %-20s %-4s err %.3g  ratio [%.4f, %.4f]  %d of %d" % (name, integrator, what, big.max(), ratio.min(), ratio.max(),
                                                                                   int(sel.sum()), N))


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", DIRECTIONAL_CHAINS)
def test_directional_consistency_with_central_differences_of_the_rollout(name, integrator):
    """Asserted: err at the larger h <= 20 x the oracle's own worst figure of the chain, direction and integrator (the table above this
    test; the margin the directional tests of test_gpu_torque_derivatives.py and test_gpu_forward_dynamics_derivatives.py take, for
    their reason: a wrong term shows at order 1), and err(h) / err(h / 2) in [3.5, 4.5] on the samples with err >= 1e-9, which are at
    least half of the batch."""
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N, T, dt = chain.getActiveJointsNumber(), 200, 8, 1e-2
    q0, dq0, tau, cq, cv, e, f, g = _directional_inputs(name, n, N, T)

    def loss(q, v, u):
        r = chain.rollout(_dev(torch, q, "sample"), _dev(torch, v, "sample"), _dev_seq(torch, u, "sample"), dt, integrator=integrator)
        assert bool((r[2] == 1).all())
        return (cq * r[0].cpu().numpy()).sum(axis=1) + (cv * r[1].cpu().numpy()).sum(axis=1)

    fw, st = _forward(torch, chain, q0, dq0, tau, dt, integrator)
    assert (st == 1).all()
    grads = _adjoint(torch, chain, fw, dt, integrator, gq_end=cq, gdq_end=cv)
    assert (grads[3] == 1).all()
    errs = _directional_errors(loss, grads[:3], q0, dq0, tau, e, f, g)
    k = INTEGRATORS.index(integrator)
    for j, what in enumerate(("x0", "tau")):
        big, small = errs[what]
        sel = big >= 1e-9
        ratio = big[sel] / small[sel]
        bound = 20.0 * DIRECTIONAL[name][j][k]
        print("%s %s %s: directional err max %.3g (bound %.3g), err ratio %.4g .. %.4g over %d samples (bounds 3.5, 4.5)"
              % (name, integrator, what, big.max(), bound, ratio.min(), ratio.max(), int(sel.sum())))
        assert big.max() <= bound, (what, float(big.max()), bound)
        assert int(sel.sum()) >= N // 2 and ratio.min() >= 3.5 and ratio.max() <= 4.5, (what, int(sel.sum()), float(ratio.min()), float(ratio.max()))


# ---- 4. failures and structure
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", ["ur10_like", "rev10", "rev14"])
def test_a_sample_that_failed_in_the_forward_call_is_nan_and_its_neighbours_are_untouched(name, integrator):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N, T, dt = chain.getActiveJointsNumber(), 130, 4, 1e-3
    q0, dq0, tau = _inputs(name, n, N, T, seed=6800)
    gq, gv, rq, rv = _seeds(n, N, T, seed=6800)
    fw, st = _forward(torch, chain, q0, dq0, tau, dt, integrator)
    clean = _adjoint(torch, chain, fw, dt, integrator, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv)
    assert (st == 1).all() and (clean[3] == 1).all()
    bad = 66
    q0b = q0.copy()
    q0b[bad, 0] = np.nan   # the forward call reports -1 for this sample and writes NaN records
    fwb, stb = _forward(torch, chain, q0b, dq0, tau, dt, integrator)
    others = np.arange(N) != bad
    assert stb[bad] == -1 and (stb[others] == 1).all() and bool(torch.isnan(fwb[3][:, bad]).all())
    got = _adjoint(torch, chain, fwb, dt, integrator, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv)
    assert got[3][bad] == -1 and (got[3][others] == 1).all()
    assert np.isnan(got[0][bad]).all() and np.isnan(got[1][bad]).all() and np.isnan(got[2][:, bad]).all()
    for x, y in zip(got[:3], clean[:3]):
        assert np.array_equal(x[..., others, :], y[..., others, :])
    # a NaN planted in one record only: NaN from that backward step on, the later steps' torque gradients stay
    tq, tdq, ttau, q_traj, dq_traj = fw
    q_traj = q_traj.clone()
    q_traj[1, bad, 0] = float("nan")   # x_2
    got = _adjoint(torch, chain, (tq, tdq, ttau, q_traj, dq_traj), dt, integrator, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv)
    assert got[3][bad] == -1 and (got[3][others] == 1).all()
    assert np.isnan(got[0][bad]).all() and np.isnan(got[1][bad]).all() and np.isnan(got[2][:3, bad]).all()
    assert np.array_equal(got[2][3, bad], clean[2][3, bad])
    for x, y in zip(got[:3], clean[:3]):
        assert np.array_equal(x[..., others, :], y[..., others, :])


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", ["panda_like", "rev14"])
def test_zero_seeds_no_steps_the_summed_torque_gradient_and_aliasing(name, integrator):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N, T, dt = chain.getActiveJointsNumber(), 65, 6, 1e-3
    q0, dq0, tau = _inputs(name, n, N, T, seed=6900)
    gq, gv, rq, rv = _seeds(n, N, T, seed=6900)
    for layout in ("sample", "element"):
        fw, st = _forward(torch, chain, q0, dq0, tau, dt, integrator, layout)
        assert (st == 1).all()
        # zero seeds (given as zeros, and left out): exactly zero gradients, status 1
        for kw in ({}, {"gq_end": np.zeros_like(gq), "gdq_end": np.zeros_like(gv), "gq_traj": np.zeros_like(rq), "gdq_traj": np.zeros_like(rv)}):
            z = _adjoint(torch, chain, fw, dt, integrator, layout, **kw)
            assert (z[3] == 1).all() and all((x == 0.0).all() for x in z[:3])
        # T = 0 copies the seeds
        tq, tdq, ttau, q_traj, dq_traj = fw
        z = _adjoint(torch, chain, (tq, tdq, ttau[:0], None, None), dt, integrator, layout, gq_end=gq, gdq_end=gv)
        assert np.array_equal(z[0], gq) and np.array_equal(z[1], gv) and z[2].shape == (0, N, n) and (z[3] == 1).all()
        # the sum over the steps: each entry a sum of T terms accumulated one by one, at most (T - 1) roundings of eps / 2 each of the partial
        # sums, which the sum of the absolute terms bounds: (T - 1) eps / 2 = 2.5 eps <= 4 eps against the exactly rounded sum
        per = _adjoint(torch, chain, fw, dt, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv)
        tot = _adjoint(torch, chain, fw, dt, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, sum_tau=True)
        assert tot[2].shape == (N, n) and np.array_equal(tot[0], per[0]) and np.array_equal(tot[1], per[1])
        exact = per[2].astype(np.longdouble).sum(axis=0)
        assert (np.abs(tot[2] - exact) <= 4 * EPS * np.abs(per[2]).sum(axis=0)).all()
        # gq0 / gdq0 written over the end seeds: the same bits
        d = lambda x: _dev_seq(torch, x, layout) if x.ndim == 3 else _dev(torch, x, layout)
        tgq, tgv = d(gq), d(gv)
        r = chain.rolloutAdjoint(tq, tdq, ttau, dt, q_traj, dq_traj, gq_end=tgq, gDq_end=tgv, gq_traj=d(rq), gDq_traj=d(rv), integrator=integrator,
                                 layout=layout, out={"gq0": tgq, "gDq0": tgv})
        assert r[0].data_ptr() == tgq.data_ptr() and r[1].data_ptr() == tgv.data_ptr()
        assert np.array_equal(_host(r[0], layout), per[0]) and np.array_equal(_host(r[1], layout), per[1])
        assert np.array_equal(_host_seq(r[2], layout), per[2])


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_chunk_size_does_not_change_the_result(integrator):
    torch = pytest.importorskip("torch")
    chain = _chain("rev14")
    n, N, T, dt = 14, 200, 3, 1e-3
    cs = _set(_specs(n), n)
    q0, dq0, tau = _inputs("rev14", n, N, T, seed=7000)
    gq, gv, rq, rv = _seeds(n, N, T, seed=7000)
    res = []
    for layout, chunk in (("sample", 0), ("sample", 64), ("element", 64)):
        fw, st = _forward(torch, chain, q0, dq0, tau, dt, integrator, layout, components=cs)
        assert (st == 1).all()
        res.append(_adjoint(torch, chain, fw, dt, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, components=cs,
                            chunk_samples=chunk))
    assert (res[0][3] == 1).all()
    for other in res[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(res[0], other))


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", ["ur10_like", "rev14"])
def test_replays_from_a_captured_graph(name, integrator):
    """one adjoint call captured on a single stream (no side branches), replayed on new inputs"""
    torch = pytest.importorskip("torch")
    from rosdyn_amd._lib import INTEGRATORS as CODES, Batch, RolloutAdjointDesc, check, lib
    chain = _chain(name)
    n, N, T, dt = chain.getActiveJointsNumber(), 200, 4, 1e-3
    q0, dq0, tau = _inputs(name, n, N, T, seed=7100)
    fw, st = _forward(torch, chain, q0, dq0, tau, dt, integrator)
    tq, tdq, ttau, q_traj, dq_traj = fw
    gq, gv = (torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(2))
    gq0, gdq0, gtau = torch.zeros_like(gq), torch.zeros_like(gq), torch.zeros_like(ttau)
    status = torch.zeros((N,), dtype=torch.int32, device="cuda")
    d = RolloutAdjointDesc()
    d.n_steps, d.integrator, d.dt = T, CODES[integrator], dt
    d.tau, d.tau_step_stride = ttau.data_ptr(), n * N
    d.q_traj, d.dq_traj, d.traj_step_stride = q_traj.data_ptr(), dq_traj.data_ptr(), n * N
    d.gq_end, d.gdq_end = gq.data_ptr(), gv.data_ptr()
    d.gq0, d.gdq0, d.gtau, d.gtau_step_stride, d.status = gq0.data_ptr(), gdq0.data_ptr(), gtau.data_ptr(), n * N, status.data_ptr()
    nbytes = lib().rdyn_rollout_adjoint_workspace_bytes(chain._h, C.byref(d), N, 64)
    ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device="cuda")

    def call(stream):
        b = Batch()
        b.n_samples, b.q, b.dq, b.ddq, b.layout, b.device, b.stream = N, tq.data_ptr(), tdq.data_ptr(), None, 0, -1, stream.cuda_stream
        check(lib().rdyn_rollout_adjoint(chain._h, C.byref(b), C.byref(d), None, 0, 64, ws.data_ptr() if nbytes else None, nbytes))

    call(torch.cuda.current_stream())   # first use outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            call(s)
    for k in range(2):
        gq.uniform_(-1, 1)
        gv.uniform_(-1, 1)
        for t in (gq0, gdq0, gtau):
            t.zero_()
        status.zero_()
        g.replay()
        torch.cuda.synchronize()
        again = chain.rolloutAdjoint(tq, tdq, ttau, dt, q_traj, dq_traj, gq_end=gq, gDq_end=gv, integrator=integrator, chunk_samples=64)
        assert torch.equal(gq0, again[0]) and torch.equal(gdq0, again[1]) and torch.equal(gtau, again[2]) and torch.equal(status, again[3])
        assert bool((status == 1).all()) and bool(gq0.abs().sum() > 0)


if __name__ == "__main__":
    import sys
    _measure_directional_on_the_oracle(sys.argv[1:] or DIRECTIONAL_CHAINS)
