"""GPU tests of rdyn_rollout_adjoint_parameters / Chain.rolloutParameterAdjoint: the adjoint of a rollout with the gradients with respect
to the inertial parameters (gpi) and the component parameters (gcomp).

1. Against a numpy recomposition: the step transposes of test_gpu_rollout_adjoint.py (_np_adjoint) over the library's own one-evaluation
   products, every product also asked for its parameter rows (Chain.getJointAccelerationParameterVjp) at the very seed: gpi, gcomp = the
   sum of those rows over products and samples.  Bound per entry: 1e-11 x the sum of the absolute values of the rows.  Only the roundings
   of the seeds (the kernel contracts the step updates into fmas) and the order of the additions separate the two sides.
2. gq0, gdq0, gtau and the status are rolloutAdjoint's, bit for bit.
3. T = 0; accumulate; two runs give the same bits; a horizon split into two chained calls, the earlier one accumulating.
4. A sample that fails in the middle of the horizon contributes nothing.
5. A captured graph.
Together with tests/test_gpu_parameter_vjp.py (the one-evaluation rows against the CPU oracle's regressor) 1 pins the horizon gradient to a
sum of verified products.
6. Central differences of the library's own rollout over Chain.withParameters(pi +- h delta): the one reference that does not depend on the
   code under test (the table and the criterion are at the test).
Not here: chains with more than 10 input joints (the call refuses them: tests/test_parameter_gradient_cabi.py).
Measured once on an MI355X: 1 at most 8e-14 of the sum of the absolute rows (rev10, RK4), the split horizon and the failed sample 2e-16."""
import numpy as np
import pytest

from _arrays import INTEGRATORS, _adjoint, _adjoint_inputs as _inputs, _dev, _dev_seq, _forward, _host, _host_seq, _seeds
from _chains import _cpair
from _components import _set, _specs
from _references import _lib_fd, _np_adjoint

pytestmark = pytest.mark.gpu
CHAINS = ["planar_2r", "ur10_like", "mixed_joints", "ur10_public_long", "rev10"]
DT = 1e-3


def _iname(name):
    return "ur10_like" if name == "ur10_permuted" else name


def _padjoint(torch, chain, fw, dt, integrator, layout="sample", gq_end=None, gdq_end=None, gq_traj=None, gdq_traj=None, **kw):
    """host arrays (gq0, gdq0, gtau, gpi, gcomp, status)"""
    d = lambda x: None if x is None else (_dev_seq(torch, x, layout) if x.ndim == 3 else _dev(torch, x, layout))
    tq, tdq, ttau, q_traj, dq_traj = fw
    r = chain.rolloutParameterAdjoint(tq, tdq, ttau, dt, q_traj, dq_traj, gq_end=d(gq_end), gDq_end=d(gdq_end), gq_traj=d(gq_traj),
                                      gDq_traj=d(gdq_traj), integrator=integrator, layout=layout, **kw)
    gtau = _host_seq(r[2], layout) if r[2].dim() == 3 else _host(r[2], layout)
    return (_host(r[0], layout), _host(r[1], layout), gtau, r[3].cpu().numpy(), None if r[4] is None else r[4].cpu().numpy(), r[5].cpu().numpy())


class _Rows(object):
    """the library's product for _np_adjoint that also adds up the parameter rows of every product it is asked for"""

    def __init__(self, torch, chain, components):
        self.torch, self.chain, self.cs = torch, chain, components
        self.pi = self.comp = self.api = self.acomp = 0.0

    def __call__(self, q, v, tau, seed):
        t = [_dev(self.torch, x, "sample") for x in (q, v, tau, seed)]
        out = self.chain.getJointAccelerationVjp(*t, components=self.cs)
        assert (out[0].cpu().numpy() == 1).all()
        rows = self.chain.getJointAccelerationParameterVjp(*t, components=self.cs)
        pi = rows[0].cpu().numpy()
        self.pi, self.api = self.pi + pi, self.api + np.abs(pi)
        if rows[1] is not None:
            comp = rows[1].cpu().numpy()
            self.comp, self.acomp = self.comp + comp, self.acomp + np.abs(comp)
        return tuple(x.cpu().numpy() for x in out[1:])


def _expected(torch, chain, cs, q0, dq0, tau, qt, vt, gq, gv, rq, rv, dt, integrator, keep=None):
    """(gpi, |gpi| terms, gcomp, |gcomp| terms) by the numpy recomposition; keep: the samples that count (None: all)"""
    rows = _Rows(torch, chain, cs)
    _np_adjoint(rows, _lib_fd(torch, chain, cs), q0, dq0, tau, qt, vt, gq, gv, dt, integrator, rq, rv)
    keep = slice(None) if keep is None else keep
    if cs is None:
        return rows.pi[keep].sum(axis=0), rows.api[keep].sum(axis=0), None, None
    return rows.pi[keep].sum(axis=0), rows.api[keep].sum(axis=0), rows.comp[keep].sum(axis=0), rows.acomp[keep].sum(axis=0)


def _within(got, want, terms, factor, what):
    err = np.abs(got - want)
    worst = float((err / np.where(terms > 0, terms, 1.0)).max())
    assert (err <= factor * terms).all(), (what, worst)
    return worst


# ---- 1., 2. the numpy recomposition; the sibling's outputs
@pytest.mark.parametrize("with_components", [False, True], ids=["plain", "components"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", CHAINS)
def test_against_the_numpy_recomposition_and_the_sibling_bitwise(name, integrator, with_components):
    torch = pytest.importorskip("torch")
    chain, _ = _cpair(name, oracle=False)
    n = chain.getActiveJointsNumber()
    cs = _set(_specs(n), n) if with_components else None
    worst = 0.0
    for N, T in ((1, 1), (63, 3), (65, 1), (130, 3)):
        q0, dq0, tau = _inputs(_iname(name), n, N, T, seed=8100 + N)
        gq, gv, rq, rv = _seeds(n, N, T, seed=8100 + N)
        got = None
        for layout in ("sample", "element"):
            fw, st = _forward(torch, chain, q0, dq0, tau, DT, integrator, layout, components=cs)
            assert (st == 1).all()
            r = _padjoint(torch, chain, fw, DT, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, components=cs)
            sib = _adjoint(torch, chain, fw, DT, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, components=cs)
            assert (r[5] == 1).all() and np.array_equal(r[5], sib[3])
            assert all(np.array_equal(x, y) for x, y in zip(r[:3], sib[:3])), "gq0, gdq0, gtau are rolloutAdjoint's bits"
            if layout == "sample":
                qt, vt = _host_seq(fw[3], layout), _host_seq(fw[4], layout)
            if got is not None:
                assert np.array_equal(got[3], r[3]) and (cs is None or np.array_equal(got[4], r[4])), "the layouts give the same bits"
            got = r
        gpi, api, gcomp, acomp = _expected(torch, chain, cs, q0, dq0, tau, qt, vt, gq, gv, rq, rv, DT, integrator)
        assert got[3].shape == (10 * chain.getJointsNumber(),) and np.isfinite(got[3]).all() and np.abs(gpi).max() > 0
        worst = max(worst, _within(got[3], gpi, api, 1e-11, ("gpi", N, T)))
        if cs is None:
            assert got[4] is None
        else:
            assert got[4].shape == (cs.columns,)
            worst = max(worst, _within(got[4], gcomp, acomp, 1e-11, ("gcomp", N, T)))
    print("%s %s %s: worst distance / sum of absolute rows %.3g (bound 1e-11)" % (name, integrator, "components" if with_components else "plain", worst))


# ---- 3. T = 0, accumulate, reproducibility, the split horizon
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", ["ur10_like", "ur10_public_long", "rev10"])
def test_no_steps_accumulation_reproducibility_and_the_split_horizon(name, integrator):
    torch = pytest.importorskip("torch")
    chain, _ = _cpair(name, oracle=False)
    n, N, T = chain.getActiveJointsNumber(), 65, 4
    cs = _set(_specs(n), n)
    P, K = 10 * chain.getJointsNumber(), cs.columns
    q0, dq0, tau = _inputs(name, n, N, T, seed=8400)
    gq, gv, rq, rv = _seeds(n, N, T, seed=8400)
    fw, st = _forward(torch, chain, q0, dq0, tau, DT, integrator, components=cs)
    assert (st == 1).all()
    tq, tdq, ttau, q_traj, dq_traj = fw
    kw = dict(gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, components=cs)
    whole = _padjoint(torch, chain, fw, DT, integrator, **kw)
    again = _padjoint(torch, chain, fw, DT, integrator, **kw)
    assert np.array_equal(whole[3], again[3]) and np.array_equal(whole[4], again[4]), "two runs, the same bits"
    # no steps: zeros, or the outputs as they were
    z = _padjoint(torch, chain, (tq, tdq, ttau[:0], None, None), DT, integrator, gq_end=gq, gdq_end=gv, components=cs)
    assert (z[3] == 0.0).all() and (z[4] == 0.0).all() and np.array_equal(z[0], gq) and np.array_equal(z[1], gv) and (z[5] == 1).all()
    keep = {"gpi": torch.full((P,), 1.5, dtype=torch.float64, device="cuda"), "gcomp": torch.full((K,), -2.0, dtype=torch.float64, device="cuda")}
    _padjoint(torch, chain, (tq, tdq, ttau[:0], None, None), DT, integrator, gq_end=gq, gdq_end=gv, components=cs, out=dict(keep), accumulate=True)
    assert bool((keep["gpi"] == 1.5).all()) and bool((keep["gcomp"] == -2.0).all())
    # accumulate adds
    _padjoint(torch, chain, fw, DT, integrator, out=dict(keep), accumulate=True, **kw)
    assert np.array_equal(keep["gpi"].cpu().numpy(), 1.5 + whole[3]) and np.array_equal(keep["gcomp"].cpu().numpy(), -2.0 + whole[4])
    # the split horizon: the later part first, the earlier part seeded by its result and adding to its gpi, gcomp
    _, api, _, acomp = _expected(torch, chain, cs, q0, dq0, tau, _host_seq(q_traj, "sample"), _host_seq(dq_traj, "sample"), gq, gv, rq, rv, DT, integrator)
    for cut in (1, 3):
        later = (q_traj[cut - 1], dq_traj[cut - 1], ttau[cut:], q_traj[cut:], dq_traj[cut:])
        b = _padjoint(torch, chain, later, DT, integrator, gq_end=gq, gdq_end=gv, gq_traj=rq[cut:], gdq_traj=rv[cut:], components=cs)
        out = {"gpi": torch.from_numpy(b[3]).cuda(), "gcomp": torch.from_numpy(b[4]).cuda()}
        earlier = (tq, tdq, ttau[:cut], q_traj[:cut], dq_traj[:cut])
        a = _padjoint(torch, chain, earlier, DT, integrator, gq_end=b[0], gdq_end=b[1], gq_traj=rq[:cut], gdq_traj=rv[:cut], components=cs,
                      out=out, accumulate=True)
        assert np.array_equal(a[0], whole[0]) and np.array_equal(a[1], whole[1])
        w = max(_within(a[3], whole[3], api, 1e-12, ("gpi", cut)), _within(a[4], whole[4], acomp, 1e-12, ("gcomp", cut)))
        print("%s %s cut %d: split against single call, worst distance / sum of absolute rows %.3g (bound 1e-12)" % (name, integrator, cut, w))
    # gq0, gdq0 and gtau are optional here: through the C call, gpi alone
    import ctypes as C
    from rosdyn_amd import _lib
    gpi = torch.zeros((P,), dtype=torch.float64, device="cuda")
    d = _lib.RolloutAdjointDesc()
    d.n_steps, d.integrator, d.dt = T, _lib.INTEGRATORS[integrator], DT
    d.tau, d.tau_step_stride = ttau.data_ptr(), n * N
    d.q_traj, d.dq_traj, d.traj_step_stride = q_traj.data_ptr(), dq_traj.data_ptr(), n * N
    tg = [_dev(torch, gq, "sample"), _dev(torch, gv, "sample"), _dev_seq(torch, rq, "sample"), _dev_seq(torch, rv, "sample")]
    d.gq_end, d.gdq_end, d.gq_traj, d.gdq_traj, d.gtraj_step_stride = tg[0].data_ptr(), tg[1].data_ptr(), tg[2].data_ptr(), tg[3].data_ptr(), n * N
    comps, n_comps = chain._component_list(cs)
    nbytes = _lib.lib().rdyn_rollout_adjoint_parameters_workspace_bytes(chain._h, C.byref(d), comps, n_comps, N, 0)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    b = _lib.Batch(N, tq.data_ptr(), tdq.data_ptr(), None, 0, -1, torch.cuda.current_stream().cuda_stream)
    pg = _lib.ParameterGradient(gpi.data_ptr(), None, 0)
    _lib.check(_lib.lib().rdyn_rollout_adjoint_parameters(chain._h, C.byref(b), C.byref(d), comps, n_comps, C.byref(pg), 0, ws.data_ptr(), nbytes))
    assert np.array_equal(gpi.cpu().numpy(), whole[3])


# ---- 4. a sample that fails in the middle of the horizon
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", ["ur10_like", "ur10_public_long"])
def test_a_sample_that_fails_mid_horizon_contributes_nothing(name, integrator):
    torch = pytest.importorskip("torch")
    chain, _ = _cpair(name, oracle=False)
    n, N, T, bad = chain.getActiveJointsNumber(), 130, 3, 70
    cs = _set(_specs(n), n)
    q0, dq0, tau = _inputs(name, n, N, T, seed=8700)
    gq, gv, rq, rv = _seeds(n, N, T, seed=8700)
    others = np.arange(N) != bad
    fw, st = _forward(torch, chain, q0, dq0, tau, DT, integrator, components=cs)
    assert (st == 1).all()
    # a NaN planted in the record of x_1 only: the backward steps 2 (and the part of 1 before the product) run clean and accumulate, then
    # the sample fails -- what it has accumulated must not count
    tq, tdq, ttau, q_traj, dq_traj = fw
    q_traj = q_traj.clone()
    q_traj[0, bad, 0] = float("nan")
    fw = (tq, tdq, ttau, q_traj, dq_traj)
    got = _padjoint(torch, chain, fw, DT, integrator, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, components=cs)
    assert got[5][bad] == -1 and (got[5][others] == 1).all() and np.isfinite(got[3]).all() and np.isfinite(got[4]).all()
    sub = lambda x: np.ascontiguousarray(x[..., others, :])
    fw2, st2 = _forward(torch, chain, sub(q0), sub(dq0), sub(tau), DT, integrator, components=cs)
    assert (st2 == 1).all()
    want = _padjoint(torch, chain, fw2, DT, integrator, gq_end=sub(gq), gdq_end=sub(gv), gq_traj=sub(rq), gdq_traj=sub(rv), components=cs)
    _, api, _, acomp = _expected(torch, chain, cs, sub(q0), sub(dq0), sub(tau), _host_seq(fw2[3], "sample"), _host_seq(fw2[4], "sample"), sub(gq),
                                 sub(gv), sub(rq), sub(rv), DT, integrator)
    w = max(_within(got[3], want[3], api, 1e-12, "gpi"), _within(got[4], want[4], acomp, 1e-12, "gcomp"))
    print("%s %s: with the failed sample against the batch without it, worst distance / sum of absolute rows %.3g (bound 1e-12)" % (name, integrator, w))


# ---- 5. a captured graph
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_replays_from_a_captured_graph(integrator):
    """one call captured on a single stream, every buffer made beforehand, replayed on new seeds"""
    torch = pytest.importorskip("torch")
    chain, _ = _cpair("ur10_like", oracle=False)
    n, N, T = chain.getActiveJointsNumber(), 130, 3
    q0, dq0, tau = _inputs("ur10_like", n, N, T, seed=8900)
    fw, st = _forward(torch, chain, q0, dq0, tau, DT, integrator)
    tq, tdq, ttau, q_traj, dq_traj = fw
    gq, gv = (torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(2))
    call = lambda: chain.rolloutParameterAdjoint(tq, tdq, ttau, DT, q_traj, dq_traj, gq_end=gq, gDq_end=gv, integrator=integrator)
    call()   # first use outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            res = call()
    for k in range(2):
        gq.uniform_(-1, 1)
        gv.uniform_(-1, 1)
        g.replay()
        torch.cuda.synchronize()
        again = call()
        for x, y in zip(res, again):
            assert (x is None and y is None) or torch.equal(x, y)
        assert bool((res[5] == 1).all()) and bool(res[3].abs().sum() > 0)


# ---- 6. central differences of the library's rollout over Chain.withParameters
# L = <c_q, q_T> + <c_v, Dq_T>, T = 8, dt = 1e-2, N = 200; delta, H, the error and its scale as tests/test_parameter_gradient_inputs.py defines
# them and measures them on the CPU oracle alone (its header has the table; ORACLE_WORST is that table):
#     chain         err(H) / scale, worst on the oracle (Euler / RK4)     samples >= 1e-9 scale
#     planar_2r     7.839e-05 / 8.097e-05                                 200 / 200 of 200
#     ur10_like     5.840e-05 / 6.196e-05                                 200 / 200 of 200
#     panda_like    4.089e-04 / 3.272e-04                                 200 / 200 of 200
# Here <gpi, delta> is the library's: per sample, from rolloutParameterAdjoint on that sample alone (the call returns sums over the samples).
# Asserted: err(H) / err(H / 2) in [3.5, 4.5] on the samples with err(H) >= 1e-9 scale, at least three quarters of the batch, and
# err(H) / scale <= 2 x the oracle's worst (the margin for the rounding difference between library and oracle: a wrong term -- a sign, a
# stage weight, parameters the companion did not get -- shows at order 1).
# Measured once on an MI355X: err(H) / scale 7.84e-5 / 8.10e-5 (planar_2r), 5.84e-5 / 6.20e-5 (ur10_like), 4.09e-4 / 3.27e-4 (panda_like) -- the
# oracle's figures to three digits --, err ratio 3.999 .. 4.004, all 200 samples qualify.
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", ["planar_2r", "ur10_like", "panda_like"])
def test_directional_consistency_with_central_differences_over_with_parameters(name, integrator):
    torch = pytest.importorskip("torch")
    from _arrays import _directional_inputs
    from _arrays import DIRECTIONAL_DT as DT_CD, DIRECTIONAL_H as H, DIRECTIONAL_N as N, DIRECTIONAL_T as T, _direction
    from _references import ORACLE_WORST
    chain, _ = _cpair(name, oracle=False)
    n = chain.getActiveJointsNumber()
    q0, dq0, tau, cq, cv = _directional_inputs(name, n, N, T)[:5]
    pi = chain.getNominalParameters()
    delta = _direction(pi)
    tq, tdq, ttau = _dev(torch, q0, "sample"), _dev(torch, dq0, "sample"), _dev_seq(torch, tau, "sample")

    def loss(p):
        r = chain.withParameters(p).rollout(tq, tdq, ttau, DT_CD, integrator=integrator)
        assert bool((r[2] == 1).all())
        return (cq * r[0].cpu().numpy()).sum(axis=1) + (cv * r[1].cpu().numpy()).sum(axis=1)

    # per sample: the gradient of that sample's loss
    tcq, tcv = _dev(torch, cq, "sample"), _dev(torch, cv, "sample")
    fw = chain.rollout(tq, tdq, ttau, DT_CD, integrator=integrator, trajectory_every=1)
    gpi = np.empty((N, pi.size))
    for s in range(N):
        one = lambda t: t[..., s:s + 1, :].contiguous()
        r = chain.rolloutParameterAdjoint(one(tq), one(tdq), one(ttau), DT_CD, one(fw[3]), one(fw[4]), gq_end=one(tcq), gDq_end=one(tcv),
                                          integrator=integrator)
        assert int(r[5][0]) == 1
        gpi[s] = r[3].cpu().numpy()
    # ... and their sum is what the batched call returns (to the rounding of the sum)
    whole = chain.rolloutParameterAdjoint(tq, tdq, ttau, DT_CD, fw[3], fw[4], gq_end=tcq, gDq_end=tcv, integrator=integrator)[3].cpu().numpy()
    assert (np.abs(whole - gpi.sum(axis=0)) <= 1e-12 * np.abs(gpi).sum(axis=0)).all()
    lin = gpi @ delta
    scale = np.abs((gpi * delta).reshape(N, -1, 10).sum(axis=2)).max(axis=1)
    errs = [np.abs((loss(pi + h * delta) - loss(pi - h * delta)) / (2.0 * h) - lin) / scale for h in (H, 0.5 * H)]
    sel = errs[0] >= 1e-9
    ratio = errs[0][sel] / errs[1][sel]
    cap = 2.0 * ORACLE_WORST[name][INTEGRATORS.index(integrator)]
    print("%s %s: directional err(H) / scale max %.3g (cap %.3g), err ratio %.4g .. %.4g over %d of %d samples (bounds 3.5, 4.5)"
          % (name, integrator, errs[0].max(), cap, ratio.min(), ratio.max(), int(sel.sum()), N))
    assert int(sel.sum()) >= 3 * N // 4 and ratio.min() >= 3.5 and ratio.max() <= 4.5, (int(sel.sum()), float(ratio.min()), float(ratio.max()))
    assert errs[0].max() <= cap, (float(errs[0].max()), cap)
