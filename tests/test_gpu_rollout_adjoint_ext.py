"""GPU tests of rdyn_rollout_adjoint_ext / Chain.rolloutAdjoint(ext_wrenches=): the exact transpose of the scheme Chain.rollout(ext_wrenches=)
integrates, with the gradient with respect to the wrenches.

1. One step against the library's own product: the numpy step transposes of test_gpu_rollout_adjoint.py run over
   getJointAccelerationVjp(ext_wrenches=) and getJointAcceleration(ext_wrenches=); gext of the step is the sum of the products' "ext".
   Bound per sample and entry: 1e-11 x the sum of the absolute terms of the entry -- the same composition on magnitudes, |matrix| |seed| for
   every product with the matrices of getJointAccelerationDerivatives at tau - tau_E, and |A|' (|M^-1| |seed|) for the wrench record (A
   the wrench-torque matrix of test_gpu_forward_dynamics_vjp_ext.py).  The terms of d tau_E / d q are left out of the magnitudes: the bound
   is the smaller for it.
2. A horizon split anywhere into two chained calls gives the single call's bits: a wrench per step, gw per step, running seeds, gtau per
   step.  The summed gw equals the sum of the per-step records to rounding.
3. Directional consistency against central differences of Chain.rollout(ext_wrenches=) along (x0, tau, wrench), see the table at the test.
4. Failures, T = 0, aliasing, the chains that are not served with wrenches, a captured graph."""
import ctypes as C

import numpy as np
import pytest

from _arrays import (EPS, INTEGRATORS, WRENCH_SCALE as SCALE, _dev, _dev_seq, _dev_w, _dev_wseq,
                     _host, _host_seq, _host_w, _mat, _seeds, _wrench_rollout_inputs as _inputs, _wrenches)
from _chains import _chain, _trio
from _components import _set, _specs
from _references import (_WrenchTorque, _input_types, _np_adjoint, _np_rollout, _np_step,
                         _np_step_adjoint, _oracle_fd_ext, _reference, _tau_e, _wrench_matrix)

pytestmark = pytest.mark.gpu
CHAINS = ["planar_2r", "mixed_joints", "ur10_like", "panda_like", "ur10_public", "ur10_permuted", "rev10"]
LAYOUTS = ("sample", "element")


def _forward(torch, chain, q0, dq0, tau, W, dt, integrator, layout="sample", link=None, seq=False, components=None):
    """device tensors of the forward call with one record per step: (tq0, tdq0, ttau, q_traj, dq_traj, tw, link name), and the host status"""
    tq, tdq, ttau = _dev(torch, q0, layout), _dev(torch, dq0, layout), _dev_seq(torch, tau, layout)
    tw = _dev_wseq(torch, W, layout) if seq else _dev_w(torch, W, layout)
    name = None if link is None else chain.getLinksName()[link]
    r = chain.rollout(tq, tdq, ttau, dt, integrator=integrator, layout=layout, trajectory_every=1, components=components, ext_wrenches=tw,
                      ext_link=name)
    return (tq, tdq, ttau, r[3], r[4], tw, name), r[2].cpu().numpy()


def _adjoint(torch, chain, fw, dt, integrator, layout="sample", gq_end=None, gdq_end=None, gq_traj=None, gdq_traj=None, **kw):
    """host arrays (gq0, gdq0, gtau, status, gext); gext (T, N, L, 6) / (T, N, 6), or one record with sum_ext"""
    d = lambda x: None if x is None else (_dev_seq(torch, x, layout) if x.ndim == 3 else _dev(torch, x, layout))
    tq, tdq, ttau, q_traj, dq_traj, tw, name = fw
    N = tq.shape[0] if layout == "sample" else tq.shape[1]
    r = chain.rolloutAdjoint(tq, tdq, ttau, dt, q_traj, dq_traj, gq_end=d(gq_end), gDq_end=d(gdq_end), gq_traj=d(gq_traj), gDq_traj=d(gdq_traj),
                             integrator=integrator, layout=layout, ext_wrenches=tw, ext_link=name, want_ext=True, **kw)
    gtau = _host_seq(r[2], layout) if r[2].dim() == 3 else _host(r[2], layout)
    ge = r[4]
    if kw.get("sum_ext"):
        gext = _host_w(ge, layout, N)
    else:
        gext = np.array([_host_w(g, layout, N) for g in ge]) if ge.shape[0] else np.zeros((0, N, 6))
    return _host(r[0], layout), _host(r[1], layout), gtau, r[3].cpu().numpy(), gext


# ---- 1. one step against the library's own product
def _lib_pieces(torch, chain, chain0, W, link, components, L):
    """fd, vjp (which adds every product's "ext" to box["g"]), and the same on magnitudes"""
    name = None if link is None else chain.getLinksName()[link]
    tw = _dev_w(torch, W, "sample")
    Wl = W
    if link is not None:
        Wl = np.zeros((len(W), L, 6))
        Wl[:, link] = W
    box = {"g": 0.0, "m": 0.0}

    def fd(q, v, tau):
        a, st = chain.getJointAcceleration(_dev(torch, q, "sample"), _dev(torch, v, "sample"), _dev(torch, tau, "sample"), components=components,
                                           ext_wrenches=tw, ext_link=name)
        assert (st.cpu().numpy() == 1).all()
        return a.cpu().numpy()

    def vjp(q, v, tau, seed):
        out = chain.getJointAccelerationVjp(*(_dev(torch, x, "sample") for x in (q, v, tau, seed)), components=components, ext_wrenches=tw,
                                            ext_link=name, want=("q", "dq", "tau", "ext"))
        assert (out[0].cpu().numpy() == 1).all()
        box["g"] = box["g"] + out[4].cpu().numpy()
        return tuple(t.cpu().numpy() for t in out[1:4])

    def avjp(q, v, tau, m):
        tau_e = _tau_e(torch, chain0, q, Wl)
        out = chain.getJointAccelerationDerivatives(*(_dev(torch, x, "sample") for x in (q, v, tau - tau_e)), components=components)
        Xq, Xv, Mi = (np.abs(_mat(t, "sample")) for t in out[2:])   # [s, i, k]
        w = np.einsum("sik,si->sk", Mi, m)
        A = np.abs(_wrench_matrix(torch, chain0, q, L))
        mag = np.einsum("sie,si->se", A, w).reshape(len(q), L, 6)
        box["m"] = box["m"] + (mag if link is None else mag[:, link])
        return np.einsum("sik,si->sk", Xq, m), np.einsum("sik,si->sk", Xv, m), w

    return fd, vjp, avjp, box


@pytest.mark.parametrize("with_components", [False, True], ids=["plain", "components"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", CHAINS)
def test_one_step_against_the_library_own_product(name, integrator, with_components):
    torch = pytest.importorskip("torch")
    chain, _, chain0 = _trio(name)
    n, L, dt = chain.getActiveJointsNumber(), chain.getLinksNumber(), 1e-3
    cs = _set(_specs(n), n) if with_components else None
    worst = 0.0
    for N in (1, 63, 64, 65, 200):
        q0, dq0, tau = _inputs(name, n, N, 1, seed=10100 + N)
        gq, gv, _, _ = _seeds(n, N, 1, seed=10100 + N)
        W_all = _wrenches(name, N, L, seed=10150 + N)
        for link in (None, L - 1, L // 2):
            W = W_all if link is None else W_all[:, link]
            fd, vjp, avjp, box = _lib_pieces(torch, chain, chain0, W, link, cs, L)
            want = _np_step_adjoint(vjp, fd, q0, dq0, tau[0], gq, gv, dt, integrator) + (box["g"],)
            mag = _np_step_adjoint(avjp, fd, q0, dq0, tau[0], np.abs(gq), np.abs(gv), dt, integrator) + (box["m"],)
            got = None
            for layout in LAYOUTS:
                fw = (_dev(torch, q0, layout), _dev(torch, dq0, layout), _dev_seq(torch, tau, layout), None, None, _dev_w(torch, W, layout),
                      None if link is None else chain.getLinksName()[link])
                r = _adjoint(torch, chain, fw, dt, integrator, layout, gq_end=gq, gdq_end=gv, components=cs)
                assert r[3].shape == (N,) and (r[3] == 1).all(), np.unique(r[3])
                if got is not None:
                    assert all(np.array_equal(x, y) for x, y in zip(got, r)), "the layouts give the same bits"
                got = r
            for what, g, w, m in zip(("gq0", "gdq0", "gtau", "gext"), (got[0], got[1], got[2][0], got[4][0]), want, mag):
                assert np.isfinite(g).all() and g.shape == w.shape
                if what != "gext":
                    assert (m > 0).all()
                else:   # the base link's record, and a link no input joint moves, are exactly 0 on both sides
                    assert (g[m == 0] == 0.0).all() and (w[m == 0] == 0.0).all()
                sel = m > 0
                ratio = float((np.abs(g - w)[sel] / m[sel]).max())
                worst = max(worst, ratio)
                assert ratio <= 1e-11, (what, N, link, ratio)
    print("%s %s %s: worst distance / sum of absolute terms %.3g (bound 1e-11)" % (name, integrator, "components" if with_components else "plain", worst))


# ---- 2. the horizon can be split anywhere, bitwise
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", CHAINS)
def test_the_horizon_can_be_split_anywhere_bitwise(name, integrator, layout):
    torch = pytest.importorskip("torch")
    chain, _, _ = _trio(name)
    n, L, N, T, dt = chain.getActiveJointsNumber(), chain.getLinksNumber(), 65, 6, 1e-3
    cs = _set(_specs(n), n)
    q0, dq0, tau = _inputs(name, n, N, T, seed=10400)
    gq, gv, rq, rv = _seeds(n, N, T, seed=10400)
    W_all = np.array([_wrenches(name, N, L, seed=10450 + t) for t in range(T)])
    for link in (None, L - 1):
        W = W_all if link is None else W_all[:, :, link]
        fw, st = _forward(torch, chain, q0, dq0, tau, W, dt, integrator, layout, link=link, seq=True, components=cs)
        assert (st == 1).all()
        tq, tdq, ttau, q_traj, dq_traj, tw, lname = fw
        whole = _adjoint(torch, chain, fw, dt, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, components=cs)
        assert (whole[3] == 1).all() and all(np.isfinite(x).all() for x in whole[:3] + whole[4:])
        assert whole[4].shape == W.shape and np.abs(whole[4]).max() > 0
        for cut in range(1, T):
            later = (q_traj[cut - 1], dq_traj[cut - 1], ttau[cut:], q_traj[cut:], dq_traj[cut:], tw[cut:], lname)
            b = _adjoint(torch, chain, later, dt, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq[cut:], gdq_traj=rv[cut:], components=cs)
            earlier = (tq, tdq, ttau[:cut], q_traj[:cut], dq_traj[:cut], tw[:cut], lname)
            a = _adjoint(torch, chain, earlier, dt, integrator, layout, gq_end=b[0], gdq_end=b[1], gq_traj=rq[:cut], gdq_traj=rv[:cut], components=cs)
            assert np.array_equal(a[0], whole[0]) and np.array_equal(a[1], whole[1]), cut
            assert np.array_equal(np.concatenate([a[2], b[2]]), whole[2]) and np.array_equal(np.concatenate([a[4], b[4]]), whole[4]), cut
            assert (a[3] == 1).all() and (b[3] == 1).all()
        # The sum over the steps against the per-step records.  Both add the same products p (one per step, RK4: four, which share their
        # sign up to O(dt): sum |p| <= 1.25 sum |record| is assumed, and is generous): the records round each step's sum (3 roundings),
        # the running sum rounds 4 T - 1 times, so the two differ by at most (4 T + 2) eps / 2 sum |p| <= 16 eps sum |record| at T = 6.
        tot = _adjoint(torch, chain, fw, dt, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, components=cs, sum_ext=True)
        assert tot[4].shape == W.shape[1:] and all(np.array_equal(x, y) for x, y in zip(tot[:4], whole[:4]))
        exact = whole[4].astype(np.longdouble).sum(axis=0)
        assert (np.abs(tot[4] - exact) <= 16 * EPS * np.abs(whole[4]).sum(axis=0)).all()
        again = _adjoint(torch, chain, fw, dt, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, components=cs, sum_ext=True)
        assert np.array_equal(again[4], tot[4]), "the summed record is reproducible bit for bit"


# ---- 3. directional consistency
# L = <c_q, q_T> + <c_v, dq_T>, T = 8, dt = 1e-2, N = 200, wrenches on every link held over the horizon (entries uniform in +- the chain's
# torque scale); the gradient of the adjoint call along (e, f) on (q0, dq0) -- h = 2^-9 and 2^-10 --, along g on tau and along k on the
# wrenches -- entries uniform in +- the torque scale, h = 2^-7 and 2^-8 -- against the central difference of Chain.rollout(ext_wrenches=)
# itself.  err = |difference| / scale per sample, scale = the largest |term| of the sample's inner product: test_gpu_rollout_adjoint.py's
# settings.  Measured on the CPU ORACLE alone with this test's own inputs (_measure_directional_on_the_oracle below: the oracle's rollout with
# wrenches of test_gpu_rollout_ext.py against the numpy adjoint with the oracle's exact matrices, d tau_E / d q by the spectral scheme and
# the wrench-torque matrix from unit wrenches); err at the larger h, worst over the samples, Euler / RK4; ratio = err at the larger h over
# err at the smaller, range over both integrators on the samples with err >= 1e-9:
#     chain         direction  err / scale, worst (Euler / RK4)     ratio              samples >= 1e-9 scale (Euler / RK4)
#     planar_2r     x0        7.19e-06 / 7.5e-06                   [3.9930, 4.0053]   199 / 200 of 200
#     planar_2r     tau       2.65e-07 / 2.86e-07                  [3.9512, 4.0294]   125 / 125 of 200
#     planar_2r     wrench    5.39e-07 / 6.09e-07                  [3.9898, 4.0141]   161 / 163 of 200
#     mixed_joints  x0        4.61e-05 / 4.66e-05                  [3.9937, 4.0349]   200 / 200 of 200
#     mixed_joints  tau       4.36e-06 / 4.43e-06                  [3.9945, 4.0049]   186 / 184 of 200
#     mixed_joints  wrench    8.27e-06 / 1.57e-05                  [3.9904, 4.0072]   187 / 187 of 200
#     ur10_like     x0        4.14e-05 / 4.43e-05                  [3.9982, 4.0016]   200 / 200 of 200
#     ur10_like     tau       6.62e-06 / 6.53e-06                  [3.9911, 4.0110]   189 / 187 of 200
#     ur10_like     wrench      0.0003 / 0.000327                  [3.9970, 4.0030]   197 / 197 of 200
#     panda_like    x0        0.000361 / 0.000383                  [3.7927, 4.0036]   200 / 200 of 200
#     panda_like    tau       4.17e-05 / 6.21e-05                  [3.9983, 4.0032]   200 / 200 of 200
#     panda_like    wrench    0.000127 / 0.000177                  [3.9963, 4.0033]   200 / 200 of 200
#     ur10_public   x0        5.74e-05 / 5.73e-05                  [3.9829, 4.0006]   200 / 200 of 200
#     ur10_public   tau       6.44e-06 / 6.98e-06                  [3.9853, 4.0281]   196 / 194 of 200
#     ur10_public   wrench    3.75e-05 / 4.35e-05                  [3.9978, 4.0012]   199 / 199 of 200
#     rev10         x0         4.5e-05 / 4.95e-05                  [3.9978, 4.0017]   200 / 200 of 200
#     rev10         tau       0.000109 / 0.000111                  [3.9963, 4.0013]   200 / 200 of 200
#     rev10         wrench    3.27e-05 / 3.68e-05                  [3.9978, 4.0005]   200 / 200 of 200
# The oracle alone meets both conditions on every chain with these settings (ratio in [3.5, 4.5] on at least half of the batch).
DIRECTIONAL_E = {
    # chain: {direction: (err Euler, err RK4)}: the table's worst figures
    "planar_2r": {"x0": (7.19e-06, 7.5e-06), "tau": (2.65e-07, 2.86e-07), "wrench": (5.39e-07, 6.09e-07)},
    "mixed_joints": {"x0": (4.61e-05, 4.66e-05), "tau": (4.36e-06, 4.43e-06), "wrench": (8.27e-06, 1.57e-05)},
    "ur10_like": {"x0": (4.14e-05, 4.43e-05), "tau": (6.62e-06, 6.53e-06), "wrench": (0.0003, 0.000327)},
    "panda_like": {"x0": (0.000361, 0.000383), "tau": (4.17e-05, 6.21e-05), "wrench": (0.000127, 0.000177)},
    "ur10_public": {"x0": (5.74e-05, 5.73e-05), "tau": (6.44e-06, 6.98e-06), "wrench": (3.75e-05, 4.35e-05)},
    "rev10": {"x0": (4.5e-05, 4.95e-05), "tau": (0.000109, 0.000111), "wrench": (3.27e-05, 3.68e-05)},
}
DIRECTIONAL_CHAINS = ["planar_2r", "mixed_joints", "ur10_like", "panda_like", "ur10_public", "rev10"]


def _directional_inputs(name, n, L, N=200, T=8):
    from rosdyn_amd.samples import uniform_pm1
    q0, dq0, tau = _inputs(name, n, N, T, seed=10700)
    cq, cv, e, f = (uniform_pm1(10710 + i, (N, n)) for i in range(4))
    key = name if name in SCALE else "ur10_like"
    g = SCALE[key] * uniform_pm1(10714, (T, N, n))
    W = _wrenches(name, N, L, seed=10715)
    k = _wrenches(name, N, L, seed=10716)
    return q0, dq0, tau, W, cq, cv, e, f, g, k


def _directional_errors(loss, grads, q0, dq0, tau, W, e, f, g, k):
    """loss(q0, dq0, tau, W) -> (N,); grads = (gq0, gdq0, gtau, gW).  {direction: (err at the larger h, err at the smaller h)} per sample"""
    gq0, gdq0, gtau, gW = grads
    N = len(q0)
    tx = np.concatenate([gq0 * e, gdq0 * f], axis=1)
    tt = np.moveaxis(gtau * g, 0, 1).reshape(N, -1)
    tw = (gW * k).reshape(N, -1)
    out = {}
    for what, terms, hs, move in (("x0", tx, (2.0 ** -9, 2.0 ** -10), lambda h: (q0 + h * e, dq0 + h * f, tau, W)),
                                  ("tau", tt, (2.0 ** -7, 2.0 ** -8), lambda h: (q0, dq0, tau + h * g, W)),
                                  ("wrench", tw, (2.0 ** -7, 2.0 ** -8), lambda h: (q0, dq0, tau, W + h * k))):
        lin, scale = terms.sum(axis=1), np.abs(terms).max(axis=1)
        out[what] = tuple(np.abs((loss(*move(h)) - loss(*move(-h))) / (2.0 * h) - lin) / scale for h in hs)
    return out


def _measure_directional_on_the_oracle(names=DIRECTIONAL_CHAINS):
    """the table above: `python tests/test_gpu_rollout_adjoint_ext.py [chain ...]` on the CPU (no GPU, no library call besides building the chain)"""
    N, T, dt = 200, 8, 1e-2
    for name in names:
        chain, ref, _ = _trio(name, oracle=True)
        types, L = _input_types(chain), chain.getLinksNumber()
        q0, dq0, tau, W, cq, cv, e, f, g, k = _directional_inputs(name, ref.n, L, N, T)
        fd = _oracle_fd_ext(ref, W)
        wt = _WrenchTorque(ref, W)
        units = np.zeros((6 * L, N, L, 6))
        for col in range(6 * L):
            units[col, :, col // 6, col % 6] = 1.0
        box = {"g": 0.0}

        def vjp(q, v, u, seed):
            M = ref.joint_inertia(q)
            zero = np.zeros_like(q)
            a = np.linalg.solve(M, (u - ref.joint_torque(q, v, zero, ext=W))[:, :, None])[:, :, 0]
            w = np.linalg.solve(M, seed[:, :, None])[:, :, 0]
            Dq, Dv, _, _ = _reference(ref, types, q, v, a)
            DE, _, _, _ = _reference(wt, types, q, v, zero)
            base = ref.joint_torque(q, zero, zero)
            A = np.stack([ref.joint_torque(q, zero, zero, ext=units[col]) - base for col in range(6 * L)], axis=2)
            box["g"] = box["g"] - np.einsum("sie,si->se", A, w).reshape(N, L, 6)
            return -np.einsum("sik,si->sk", Dq + DE, w), -np.einsum("sik,si->sk", Dv, w), w

        for integrator in INTEGRATORS:
            q, v, qs, vs = q0, dq0, [], []
            for t in range(T):
                q, v = _np_step(fd, q, v, tau[t], dt, integrator)
                qs.append(q)
                vs.append(v)
            box["g"] = 0.0
            grads = _np_adjoint(vjp, fd, q0, dq0, tau, np.array(qs), np.array(vs), cq, cv, dt, integrator) + (box["g"],)

            def loss(a, b, u, w):
                qe, ve = _np_rollout(_oracle_fd_ext(ref, w), a, b, u, dt, T, integrator)
                return (cq * qe).sum(axis=1) + (cv * ve).sum(axis=1)

            for what, (big, small) in _directional_errors(loss, grads, q0, dq0, tau, W, e, f, g, k).items():
                sel = big >= 1e-9
                ratio = big[sel] / small[sel]
                print("%-14s %-20s %-6s err %.3g  ratio [%.4f, %.4f]  %d of %d" % (name, integrator, what, big.max(), ratio.min(), ratio.max(),
                                                                                   int(sel.sum()), N), flush=True)


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", DIRECTIONAL_CHAINS)
def test_directional_consistency_with_central_differences_of_the_rollout(name, integrator):
    """Asserted: err at the larger h <= 2 x the oracle's own worst figure of the chain, direction and integrator (DIRECTIONAL_E), and
    err(h) / err(h / 2) in [3.5, 4.5] on the samples with err >= 1e-9, which are at least half of the batch."""
    torch = pytest.importorskip("torch")
    chain, _, _ = _trio(name)
    n, L, N, T, dt = chain.getActiveJointsNumber(), chain.getLinksNumber(), 200, 8, 1e-2
    q0, dq0, tau, W, cq, cv, e, f, g, k = _directional_inputs(name, n, L, N, T)

    def loss(q, v, u, w):
        r = chain.rollout(_dev(torch, q, "sample"), _dev(torch, v, "sample"), _dev_seq(torch, u, "sample"), dt, integrator=integrator,
                          ext_wrenches=_dev_w(torch, w, "sample"))
        assert bool((r[2] == 1).all())
        return (cq * r[0].cpu().numpy()).sum(axis=1) + (cv * r[1].cpu().numpy()).sum(axis=1)

    fw, st = _forward(torch, chain, q0, dq0, tau, W, dt, integrator)
    assert (st == 1).all()
    grads = _adjoint(torch, chain, fw, dt, integrator, gq_end=cq, gdq_end=cv, sum_ext=True)
    assert (grads[3] == 1).all()
    errs = _directional_errors(loss, grads[:3] + grads[4:], q0, dq0, tau, W, e, f, g, k)
    j = INTEGRATORS.index(integrator)
    for what in ("x0", "tau", "wrench"):
        big, small = errs[what]
        sel = big >= 1e-9
        ratio = big[sel] / small[sel]
        bound = 2.0 * DIRECTIONAL_E[name][what][j]
        print("%s %s %s: directional err max %.3g (bound %.3g), err ratio %.4g .. %.4g over %d samples (bounds 3.5, 4.5)"
              % (name, integrator, what, big.max(), bound, ratio.min(), ratio.max(), int(sel.sum())))
        assert big.max() <= bound, (what, float(big.max()), bound)
        assert int(sel.sum()) >= N // 2 and ratio.min() >= 3.5 and ratio.max() <= 4.5, (what, int(sel.sum()), float(ratio.min()), float(ratio.max()))


# ---- 4. failures, boundaries, capture
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", ["ur10_like", "mixed_joints", "rev10"])
def test_a_sample_that_failed_in_the_forward_call_is_nan_in_its_own_outputs_only(name, integrator):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, L, N, T, dt = chain.getActiveJointsNumber(), chain.getLinksNumber(), 130, 4, 1e-3
    q0, dq0, tau = _inputs(name, n, N, T, seed=10800)
    gq, gv, rq, rv = _seeds(n, N, T, seed=10800)
    W = np.array([_wrenches(name, N, L, seed=10850 + t) for t in range(T)])
    bad, others = 66, np.arange(N) != 66
    for link in (None, L - 1):
        Wg = W if link is None else W[:, :, link]
        fw, st = _forward(torch, chain, q0, dq0, tau, Wg, dt, integrator, link=link, seq=True)
        kw = dict(gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv)
        clean = _adjoint(torch, chain, fw, dt, integrator, **kw)
        clean_sum = _adjoint(torch, chain, fw, dt, integrator, sum_ext=True, **kw)
        assert (st == 1).all() and (clean[3] == 1).all()
        q0b = q0.copy()
        q0b[bad, 0] = np.nan   # the forward call reports -1 for this sample and writes NaN records
        fwb, stb = _forward(torch, chain, q0b, dq0, tau, Wg, dt, integrator, link=link, seq=True)
        assert stb[bad] == -1 and (stb[others] == 1).all()
        for ref_out, extra in ((clean, {}), (clean_sum, {"sum_ext": True})):
            got = _adjoint(torch, chain, fwb, dt, integrator, **kw, **extra)
            assert got[3][bad] == -1 and (got[3][others] == 1).all()
            assert np.isnan(got[0][bad]).all() and np.isnan(got[1][bad]).all() and np.isnan(got[2][:, bad]).all()
            assert np.isnan(got[4][..., bad, :, :] if link is None else got[4][..., bad, :]).all()
            for x, y in zip(got[:3], ref_out[:3]):
                assert np.array_equal(x[..., others, :], y[..., others, :])
            sel = (Ellipsis, others, slice(None), slice(None)) if link is None else (Ellipsis, others, slice(None))
            assert np.array_equal(got[4][sel], ref_out[4][sel])
        # a NaN planted in the wrench of step 1 only: NaN from that backward step on, the later steps' records stay
        tq, tdq, ttau, q_traj, dq_traj, tw, lname = fw
        twb = tw.clone()
        if link is None:
            twb[1, bad, L - 1, 2] = float("nan")
        else:
            twb[1, bad, 2] = float("nan")
        got = _adjoint(torch, chain, (tq, tdq, ttau, q_traj, dq_traj, twb, lname), dt, integrator, **kw)
        assert got[3][bad] == -1 and (got[3][others] == 1).all()
        assert np.isnan(got[0][bad]).all() and np.isnan(got[2][:2, bad]).all() and np.isnan(got[4][:2, bad]).all()
        assert np.array_equal(got[2][2:, bad], clean[2][2:, bad]) and np.array_equal(got[4][2:, bad], clean[4][2:, bad])
        for x, y in zip(got[:3] + got[4:], clean[:3] + clean[4:]):
            assert np.array_equal(x[:, others] if x.ndim > 2 else x[others], y[:, others] if y.ndim > 2 else y[others])


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", ["panda_like", "ur10_public"])
def test_no_steps_zero_seeds_and_aliasing(name, integrator):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, L, N, T, dt = chain.getActiveJointsNumber(), chain.getLinksNumber(), 65, 5, 1e-3
    q0, dq0, tau = _inputs(name, n, N, T, seed=10900)
    gq, gv, rq, rv = _seeds(n, N, T, seed=10900)
    W = _wrenches(name, N, L, seed=10950)
    for layout in LAYOUTS:
        fw, st = _forward(torch, chain, q0, dq0, tau, W, dt, integrator, layout)
        assert (st == 1).all()
        tq, tdq, ttau, q_traj, dq_traj, tw, lname = fw
        # zero seeds: exactly zero gradients, the wrench gradient included
        z = _adjoint(torch, chain, fw, dt, integrator, layout)
        assert (z[3] == 1).all() and all((x == 0.0).all() for x in z[:3] + z[4:]) and z[4].shape == (T, N, L, 6)
        # T = 0 copies the seeds; no wrench record per step, and a summed record of zeros
        none = (tq, tdq, ttau[:0], None, None, tw, lname)
        z = _adjoint(torch, chain, none, dt, integrator, layout, gq_end=gq, gdq_end=gv)
        assert np.array_equal(z[0], gq) and np.array_equal(z[1], gv) and z[2].shape == (0, N, n) and z[4].shape[0] == 0 and (z[3] == 1).all()
        z = _adjoint(torch, chain, none, dt, integrator, layout, gq_end=gq, gdq_end=gv, sum_ext=True)
        assert np.array_equal(z[0], gq) and z[4].shape == (N, L, 6) and (z[4] == 0.0).all()
        # gq0 / gdq0 written over the end seeds: the same bits
        per = _adjoint(torch, chain, fw, dt, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv)
        d = lambda x: _dev_seq(torch, x, layout) if x.ndim == 3 else _dev(torch, x, layout)
        tgq, tgv = d(gq), d(gv)
        r = chain.rolloutAdjoint(tq, tdq, ttau, dt, q_traj, dq_traj, gq_end=tgq, gDq_end=tgv, gq_traj=d(rq), gDq_traj=d(rv), integrator=integrator,
                                 layout=layout, out={"gq0": tgq, "gDq0": tgv}, ext_wrenches=tw, want_ext=True)
        assert r[0].data_ptr() == tgq.data_ptr() and r[1].data_ptr() == tgv.data_ptr() and len(r) == 5
        assert np.array_equal(_host(r[0], layout), per[0]) and np.array_equal(_host(r[1], layout), per[1])
        assert np.array_equal(_host_seq(r[2], layout), per[2])
        assert np.array_equal(np.array([_host_w(g, layout, N) for g in r[4]]), per[4])
        # without want_ext the tuple is the existing one
        r4 = chain.rolloutAdjoint(tq, tdq, ttau, dt, q_traj, dq_traj, gq_end=d(gq), gDq_end=d(gv), gq_traj=d(rq), gDq_traj=d(rv),
                                  integrator=integrator, layout=layout, ext_wrenches=tw)
        assert len(r4) == 4 and np.array_equal(_host(r4[0], layout), per[0]) and np.array_equal(_host_seq(r4[2], layout), per[2])


@pytest.mark.parametrize("name", ["rev14", "ur10_public_long"])
def test_chains_on_the_chunked_route_are_unsupported_with_wrenches_and_unchanged_without(name):
    torch = pytest.importorskip("torch")
    from rosdyn_amd._lib import Batch, ExtWrenches, INTEGRATORS as CODES, RdynError, RolloutAdjointDesc, check, lib
    chain = _chain(name)
    n, L, N, T, dt = chain.getActiveJointsNumber(), chain.getLinksNumber(), 65, 3, 1e-3
    q0, dq0, tau = _inputs(name, n, N, T, seed=11000)
    gq, gv, _, _ = _seeds(n, N, T, seed=11000)
    W = _wrenches(name, N, L, seed=11001)
    for integrator in INTEGRATORS:
        fw, st = _forward(torch, chain, q0, dq0, tau, W, dt, integrator)   # the forward call serves them
        assert (st == 1).all()
        tq, tdq, ttau, q_traj, dq_traj, tw, _ = fw
        tgq, tgv = _dev(torch, gq, "sample"), _dev(torch, gv, "sample")
        for kw in ({"ext_wrenches": tw}, {"ext_wrenches": tw[:, L - 1].contiguous(), "ext_link": chain.getLinksName()[-1]}):
            with pytest.raises(RdynError, match="not served yet") as err:
                chain.rolloutAdjoint(tq, tdq, ttau, dt, q_traj, dq_traj, gq_end=tgq, gDq_end=tgv, integrator=integrator, want_ext=True, **kw)
            assert err.value.status == 5 and "chunked route" in err.value.message
            with pytest.raises(RdynError, match="not served yet") as err:
                chain.getJointAccelerationVjp(tq, tdq, ttau[0], tgq, want=("q", "ext"), **kw)
            assert err.value.status == 5
        # without wrenches: the new entry gives the base call's bits
        plain = chain.rollout(tq, tdq, ttau, dt, integrator=integrator, trajectory_every=1)
        old = chain.rolloutAdjoint(tq, tdq, ttau, dt, plain[3], plain[4], gq_end=tgq, gDq_end=tgv, integrator=integrator)
        gq0, gdq0, gtau = torch.full_like(tq, 777.0), torch.full_like(tq, 777.0), torch.full_like(ttau, 777.0)
        status = torch.zeros((N,), dtype=torch.int32, device="cuda")
        d = RolloutAdjointDesc()
        d.n_steps, d.integrator, d.dt = T, CODES[integrator], dt
        d.tau, d.tau_step_stride = ttau.data_ptr(), n * N
        d.q_traj, d.dq_traj, d.traj_step_stride = plain[3].data_ptr(), plain[4].data_ptr(), n * N
        d.gq_end, d.gdq_end = tgq.data_ptr(), tgv.data_ptr()
        d.gq0, d.gdq0, d.gtau, d.gtau_step_stride, d.status = gq0.data_ptr(), gdq0.data_ptr(), gtau.data_ptr(), n * N, status.data_ptr()
        no_w = ExtWrenches()
        no_w.w, no_w.link, no_w.step_stride = None, 99, -4   # without w nothing else of it is read
        b = Batch()
        b.n_samples, b.q, b.dq, b.ddq, b.layout, b.device = N, tq.data_ptr(), tdq.data_ptr(), None, 0, -1
        b.stream = torch.cuda.current_stream().cuda_stream
        for px in (None, C.byref(no_w)):
            nbytes = lib().rdyn_rollout_adjoint_ext_workspace_bytes(chain._h, C.byref(d), px, N, 0)
            assert nbytes == lib().rdyn_rollout_adjoint_workspace_bytes(chain._h, C.byref(d), N, 0)
            ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device="cuda")
            check(lib().rdyn_rollout_adjoint_ext(chain._h, C.byref(b), C.byref(d), None, 0, px, None, 0, ws.data_ptr() if nbytes else None, nbytes))
            assert torch.equal(gq0, old[0]) and torch.equal(gdq0, old[1]) and torch.equal(gtau, old[2]) and torch.equal(status, old[3])


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", ["ur10_like", "rev10"])
def test_replays_from_a_captured_graph(name, integrator):
    """one adjoint call captured on a single stream (no side branches), replayed on new inputs"""
    torch = pytest.importorskip("torch")
    from rosdyn_amd._lib import INTEGRATORS as CODES, Batch, ExtWrenches, ExtWrenchGradient, RolloutAdjointDesc, check, lib
    chain = _chain(name)
    n, L, N, T, dt = chain.getActiveJointsNumber(), chain.getLinksNumber(), 200, 4, 1e-3
    q0, dq0, tau = _inputs(name, n, N, T, seed=11100)
    W = np.array([_wrenches(name, N, L, seed=11150 + t) for t in range(T)])
    fw, st = _forward(torch, chain, q0, dq0, tau, W, dt, integrator, seq=True)
    tq, tdq, ttau, q_traj, dq_traj, tw, _ = fw
    gq, gv = (torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(2))
    gq0, gdq0, gtau, gw = torch.zeros_like(gq), torch.zeros_like(gq), torch.zeros_like(ttau), torch.zeros_like(tw)
    status = torch.zeros((N,), dtype=torch.int32, device="cuda")
    d = RolloutAdjointDesc()
    d.n_steps, d.integrator, d.dt = T, CODES[integrator], dt
    d.tau, d.tau_step_stride = ttau.data_ptr(), n * N
    d.q_traj, d.dq_traj, d.traj_step_stride = q_traj.data_ptr(), dq_traj.data_ptr(), n * N
    d.gq_end, d.gdq_end = gq.data_ptr(), gv.data_ptr()
    d.gq0, d.gdq0, d.gtau, d.gtau_step_stride, d.status = gq0.data_ptr(), gdq0.data_ptr(), gtau.data_ptr(), n * N, status.data_ptr()
    x, g = ExtWrenches(), ExtWrenchGradient()
    x.w, x.link, x.step_stride = tw.data_ptr(), -1, 6 * L * N
    g.gw, g.step_stride = gw.data_ptr(), 6 * L * N
    assert lib().rdyn_rollout_adjoint_ext_workspace_bytes(chain._h, C.byref(d), C.byref(x), N, 0) == 0

    def call(stream):
        b = Batch()
        b.n_samples, b.q, b.dq, b.ddq, b.layout, b.device, b.stream = N, tq.data_ptr(), tdq.data_ptr(), None, 0, -1, stream.cuda_stream
        check(lib().rdyn_rollout_adjoint_ext(chain._h, C.byref(b), C.byref(d), None, 0, C.byref(x), C.byref(g), 0, None, 0))

    call(torch.cuda.current_stream())   # first use outside capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            call(s)
    for _ in range(2):
        gq.uniform_(-1, 1)
        gv.uniform_(-1, 1)
        for t in (gq0, gdq0, gtau, gw):
            t.zero_()
        status.zero_()
        graph.replay()
        torch.cuda.synchronize()
        again = chain.rolloutAdjoint(tq, tdq, ttau, dt, q_traj, dq_traj, gq_end=gq, gDq_end=gv, integrator=integrator, ext_wrenches=tw, want_ext=True)
        assert torch.equal(gq0, again[0]) and torch.equal(gdq0, again[1]) and torch.equal(gtau, again[2]) and torch.equal(status, again[3])
        assert torch.equal(gw, again[4]) and bool((status == 1).all()) and bool(gw.abs().sum() > 0)


if __name__ == "__main__":
    import sys
    _measure_directional_on_the_oracle(sys.argv[1:] or DIRECTIONAL_CHAINS)
