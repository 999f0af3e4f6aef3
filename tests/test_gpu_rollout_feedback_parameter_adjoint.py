"""GPU tests of rdyn_rollout_adjoint_feedback_parameters / Chain.rolloutParameterAdjoint(feedback=): the adjoint of a closed-loop rollout
with the gradients with respect to the inertial parameters (gpi) and the component parameters (gcomp).

1. Against a numpy recomposition: the closed-loop adjoint of _feedback_adjoint.py (_np_fb_adjoint) over the library's own one-evaluation
   products, every product also asked for its parameter rows (Chain.getJointAccelerationParameterVjp) at the command and the very seed:
   gpi, gcomp = the sum of those rows over products and samples.  Bound per entry: 1e-11 x the sum of the absolute values of the rows
   (the open-loop test's bound).  With limits from _limits the forward call's command record shows 20 - 80 % of the commands clamped.
2. gq0, gdq0, gtau, the status and every law gradient are rolloutAdjoint(feedback=)'s, bit for bit; feedback=None is today's
   rolloutParameterAdjoint, bit for bit.
3. T = 0; two runs give the same bits; a horizon split into two chained calls, the earlier one accumulating.
4. A sample that fails in the middle of the horizon (a NaN reference) contributes nothing.
5. A captured graph.
6. Central differences of the library's own closed-loop rollout over Chain.withParameters(pi +- h delta), without limits.
7. ... with limits under hold = 1, over the samples whose clamp pattern does not change.
The tables and the criteria of 6 and 7 are in _feedback_parameters.py; test_rollout_feedback_parameter_adjoint_inputs.py re-measures them."""
import numpy as np
import pytest

from _arrays import DT, _dev, _dev_seq, _direction, _host_seq, _seeds, _wrench_rollout_inputs as _inputs
from _chains import _chain
from _components import _set, _specs
from _feedback import Law
from _feedback_adjoint import _fb_adjoint, _fb_forward, _feedback_of, _law, _loss_terms, _same_pattern
from _feedback_parameters import (CD_CHAINS, CD_H, FBP_LIMIT_NOISE, FBP_LIMIT_STEP, FBP_ORACLE_WORST, LIMIT_MODES, MODES, _case, _clamped_share,
                                  _expected, _fbp_adjoint, _within)

pytestmark = pytest.mark.gpu
CHAINS = ["planar_2r", "ur10_like", "mixed_joints", "ur10_public_long", "rev10"]
MODE_IDS = ["euler", "rk4-hold", "rk4-continuous"]
SHARED = ("gq0", "gdq0", "gtau", "status", "gq_ref", "gdq_ref", "gkp", "gkd", "glim")
# per-sample gains, limits, components
VARIANTS = {"shared": (False, False, False), "shared_limits_components": (False, True, True), "per_sample_limits": (True, True, False),
            "per_sample_components": (True, False, True)}


def _same(a, b, keys):
    return all(np.array_equal(a[k], b[k]) for k in keys if k in a or k in b)


# ---- 1., 2. the numpy recomposition; the siblings' outputs
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", CHAINS)
def test_against_the_numpy_recomposition_and_the_siblings_bitwise(name, mode, variant):
    torch = pytest.importorskip("torch")
    integrator, hold = mode
    per_sample, limits, with_components = VARIANTS[variant]
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    cs = _set(_specs(n), n) if with_components else None
    worst, clamped, commands = 0.0, 0, 0
    for N, T in ((1, 1), (63, 3), (65, 1), (130, 3)):
        q0, dq0, tau = _inputs(name, n, N, T, seed=14100 + N)
        gq, gv, rq, rv = _seeds(n, N, T, seed=14100 + N)
        gu = _seeds(n, N, T, seed=14150 + N)[2]
        law = _law(name, n, N, T, 14100 + N, per_sample, limits, q0=q0, dq0=dq0, tau=tau)
        kw = dict(gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, gu=gu, components=cs)
        got = None
        for layout in ("sample", "element"):
            fw, st, u = _fb_forward(torch, chain, q0, dq0, law, integrator, hold, layout, components=cs)
            assert (st == 1).all()
            r = _fbp_adjoint(torch, chain, fw, integrator, layout, **kw)
            sib = _fb_adjoint(torch, chain, fw, integrator, layout, **kw)
            assert (r["status"] == 1).all()
            assert all(k in r for k in sib) and _same(r, sib, SHARED), "the closed-loop adjoint's bits"
            if layout == "sample":
                qt, vt = _host_seq(fw[3], layout), _host_seq(fw[4], layout)
                if limits:
                    clamped, commands = clamped + int((np.abs(u) == law.lim).sum()), commands + u.size
            if got is not None:
                assert np.array_equal(got["gpi"], r["gpi"]) and (cs is None or np.array_equal(got["gcomp"], r["gcomp"])), "the layouts give the same bits"
            got = r
        gpi, api, gcomp, acomp = _expected(torch, chain, cs, law, q0, dq0, qt, vt, T, gq, gv, rq, rv, gu, integrator, hold)
        assert got["gpi"].shape == (10 * chain.getJointsNumber(),) and np.isfinite(got["gpi"]).all() and np.abs(gpi).max() > 0
        worst = max(worst, _within(got["gpi"], gpi, api, 1e-11, ("gpi", N, T)))
        if cs is None:
            assert got["gcomp"] is None
        else:
            assert got["gcomp"].shape == (cs.columns,)
            worst = max(worst, _within(got["gcomp"], gcomp, acomp, 1e-11, ("gcomp", N, T)))
    share = clamped / max(commands, 1)
    print("%s %s %s: worst distance / sum of absolute rows %.3g (bound 1e-11), %.1f %% of the commands clamped"
          % (name, MODE_IDS[MODES.index(mode)], variant, worst, 100.0 * share))
    if limits:
        assert 0.2 <= share <= 0.8, share


@pytest.mark.parametrize("integrator", ["semi_implicit_euler", "rk4"])
@pytest.mark.parametrize("name", ["ur10_like", "ur10_public_long"])
def test_without_a_law_every_output_is_the_open_loop_call(name, integrator):
    torch = pytest.importorskip("torch")
    import ctypes as C
    from rosdyn_amd import _lib
    from _arrays import _forward
    chain = _chain(name)
    n, N, T = chain.getActiveJointsNumber(), 65, 3
    cs = _set(_specs(n), n)
    P, K = 10 * chain.getJointsNumber(), cs.columns
    q0, dq0, tau = _inputs(name, n, N, T, seed=14200)
    gq, gv, rq, rv = _seeds(n, N, T, seed=14200)
    (tq, tdq, ttau, q_traj, dq_traj), st = _forward(torch, chain, q0, dq0, tau, DT, integrator, components=cs)
    assert (st == 1).all()
    tg = [_dev(torch, gq, "sample"), _dev(torch, gv, "sample"), _dev_seq(torch, rq, "sample"), _dev_seq(torch, rv, "sample")]
    want = chain.rolloutParameterAdjoint(tq, tdq, ttau, DT, q_traj, dq_traj, gq_end=tg[0], gDq_end=tg[1], gq_traj=tg[2], gDq_traj=tg[3],
                                         integrator=integrator, components=cs)
    # the new entry point with fb == NULL and no wrenches
    outs = [torch.full_like(tq, 7.0), torch.full_like(tq, 7.0), torch.full_like(ttau, 7.0), torch.full((P,), 7.0, dtype=torch.float64, device="cuda"),
            torch.full((K,), 7.0, dtype=torch.float64, device="cuda")]
    status = torch.zeros((N,), dtype=torch.int32, device="cuda")
    d = _lib.RolloutAdjointDesc()
    d.n_steps, d.integrator, d.dt = T, _lib.INTEGRATORS[integrator], DT
    d.tau, d.tau_step_stride = ttau.data_ptr(), n * N
    d.q_traj, d.dq_traj, d.traj_step_stride = q_traj.data_ptr(), dq_traj.data_ptr(), n * N
    d.gq_end, d.gdq_end, d.gq_traj, d.gdq_traj, d.gtraj_step_stride = tg[0].data_ptr(), tg[1].data_ptr(), tg[2].data_ptr(), tg[3].data_ptr(), n * N
    d.gq0, d.gdq0, d.gtau, d.gtau_step_stride, d.status = outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), n * N, status.data_ptr()
    comps, n_comps = chain._component_list(cs)
    nbytes = _lib.lib().rdyn_rollout_adjoint_feedback_parameters_workspace_bytes(chain._h, C.byref(d), comps, n_comps, None, None, N, 0)
    assert nbytes == _lib.lib().rdyn_rollout_adjoint_parameters_workspace_bytes(chain._h, C.byref(d), comps, n_comps, N, 0) > 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    b = _lib.Batch(N, tq.data_ptr(), tdq.data_ptr(), None, 0, -1, torch.cuda.current_stream().cuda_stream)
    pg = _lib.ParameterGradient(outs[3].data_ptr(), outs[4].data_ptr(), 0)
    _lib.check(_lib.lib().rdyn_rollout_adjoint_feedback_parameters(chain._h, C.byref(b), C.byref(d), comps, n_comps, None, None, None, None,
                                                                   C.byref(pg), 0, ws.data_ptr(), nbytes))
    for got, w in zip(outs + [status], want[:5] + (want[5],)):
        assert torch.equal(got, w)
    gf = _lib.FeedbackGradient()
    gf.gkp = outs[0].data_ptr()
    assert _lib.lib().rdyn_rollout_adjoint_feedback_parameters(chain._h, C.byref(b), C.byref(d), comps, n_comps, None, None, None, C.byref(gf),
                                                               C.byref(pg), 0, ws.data_ptr(), nbytes) == 1


# ---- 3. T = 0, reproducibility, the split horizon
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["ur10_like", "ur10_public_long", "rev10"])
def test_no_steps_reproducibility_and_the_split_horizon(name, mode):
    torch = pytest.importorskip("torch")
    integrator, hold = mode
    chain = _chain(name)
    n, N, T = chain.getActiveJointsNumber(), 65, 4
    cs = _set(_specs(n), n)
    P, K = 10 * chain.getJointsNumber(), cs.columns
    q0, dq0, tau = _inputs(name, n, N, T, seed=14400)
    gq, gv, rq, rv = _seeds(n, N, T, seed=14400)
    gu = _seeds(n, N, T, seed=14420)[3]
    law = _law(name, n, N, T, 14400, per_sample=True, limits=True, q0=q0, dq0=dq0, tau=tau)
    fw, st, _ = _fb_forward(torch, chain, q0, dq0, law, integrator, hold, components=cs)
    assert (st == 1).all()
    tq, tdq, ttau, q_traj, dq_traj, fb = fw[:6]
    kw = dict(gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, gu=gu, components=cs)
    whole = _fbp_adjoint(torch, chain, fw, integrator, **kw)
    again = _fbp_adjoint(torch, chain, fw, integrator, **kw)
    assert all(np.array_equal(whole[k], again[k]) for k in whole), "two runs, the same bits"
    assert (whole["status"] == 1).all() and np.abs(whole["gpi"]).max() > 0 and np.abs(whole["gcomp"]).max() > 0
    # no steps: zeros in gpi / gcomp and the law's sums, the end seeds copied; or, accumulating, the outputs as they were
    none = (tq, tdq, ttau[:0], None, None, fb)   # (references may be longer than the horizon)
    z = _fbp_adjoint(torch, chain, none, integrator, gq_end=gq, gdq_end=gv, components=cs)
    assert (z["gpi"] == 0.0).all() and (z["gcomp"] == 0.0).all() and np.array_equal(z["gq0"], gq) and np.array_equal(z["gdq0"], gv)
    assert (z["status"] == 1).all() and all((z[k] == 0.0).all() for k in ("gkp", "gkd", "glim"))
    shape = tuple(tq.shape)
    keep = {"gpi": torch.full((P,), 1.5, dtype=torch.float64, device="cuda"), "gcomp": torch.full((K,), -2.0, dtype=torch.float64, device="cuda")}
    keep.update({k: torch.full(shape, 5.0, dtype=torch.float64, device="cuda") for k in ("gkp", "gkd", "gtau_limit")})
    _fbp_adjoint(torch, chain, none, integrator, gq_end=gq, gdq_end=gv, components=cs, out=dict(keep), accumulate=True)
    assert bool((keep["gpi"] == 1.5).all()) and bool((keep["gcomp"] == -2.0).all()) and all(bool((keep[k] == 5.0).all()) for k in ("gkp", "gkd", "gtau_limit"))
    # the split horizon: the later part first, the earlier part seeded by its result and adding to its sums
    _, api, _, acomp = _expected(torch, chain, cs, law, q0, dq0, _host_seq(q_traj, "sample"), _host_seq(dq_traj, "sample"), T, gq, gv, rq, rv, gu,
                                 integrator, hold)
    for cut in (1, 3):
        sums = {k: torch.full(shape, 5.0, dtype=torch.float64, device="cuda") for k in ("gkp", "gkd", "gtau_limit")}
        later_law = Law(law.tau_ff[cut:], law.q_ref[cut:], law.kp, law.kd, law.dq_ref[cut:], law.lim)
        later = (q_traj[cut - 1], dq_traj[cut - 1], ttau[cut:], q_traj[cut:], dq_traj[cut:], _feedback_of(torch, later_law, "sample", hold))
        b = _fbp_adjoint(torch, chain, later, integrator, gq_end=gq, gdq_end=gv, gq_traj=rq[cut:], gdq_traj=rv[cut:], gu=gu[cut:], components=cs,
                         out=dict(sums))
        sums.update(gpi=torch.from_numpy(b["gpi"]).cuda(), gcomp=torch.from_numpy(b["gcomp"]).cuda())
        earlier_law = Law(law.tau_ff[:cut], law.q_ref[:cut], law.kp, law.kd, law.dq_ref[:cut], law.lim)
        earlier = (tq, tdq, ttau[:cut], q_traj[:cut], dq_traj[:cut], _feedback_of(torch, earlier_law, "sample", hold))
        a = _fbp_adjoint(torch, chain, earlier, integrator, gq_end=b["gq0"], gdq_end=b["gdq0"], gq_traj=rq[:cut], gdq_traj=rv[:cut], gu=gu[:cut],
                         components=cs, out=dict(sums), accumulate=True)
        assert (a["status"] == 1).all() and (b["status"] == 1).all()
        assert _same(a, whole, ("gq0", "gdq0", "gkp", "gkd", "glim")), cut
        assert all(np.array_equal(np.concatenate([a[k], b[k]]), whole[k]) for k in ("gtau", "gq_ref", "gdq_ref")), cut
        w = max(_within(a["gpi"], whole["gpi"], api, 1e-11, ("gpi", cut)), _within(a["gcomp"], whole["gcomp"], acomp, 1e-11, ("gcomp", cut)))
        print("%s %s cut %d: split against single call, worst distance / sum of absolute rows %.3g (bound 1e-11)" % (name, MODE_IDS[MODES.index(mode)], cut, w))


# ---- 4. a sample that fails in the middle of the horizon
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["ur10_like", "ur10_public_long"])
def test_a_sample_that_fails_mid_horizon_contributes_nothing(name, mode):
    torch = pytest.importorskip("torch")
    integrator, hold = mode
    chain = _chain(name)
    n, N, T, bad = chain.getActiveJointsNumber(), 130, 3, 70
    cs = _set(_specs(n), n)
    q0, dq0, tau = _inputs(name, n, N, T, seed=14700)
    gq, gv, rq, rv = _seeds(n, N, T, seed=14700)
    law = _law(name, n, N, T, 14700, per_sample=True, limits=True, q0=q0, dq0=dq0, tau=tau)
    others = np.arange(N) != bad
    fw, st, _ = _fb_forward(torch, chain, q0, dq0, law, integrator, hold, components=cs)
    assert (st == 1).all()
    kw = dict(gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, components=cs)
    clean = _fbp_adjoint(torch, chain, fw, integrator, **kw)
    # a NaN reference at step 1 of one sample, planted after the forward call: the backward step 2 runs clean and accumulates, then the
    # sample fails -- what it has accumulated must not count
    q_ref = law.q_ref.copy()
    q_ref[1, bad, 0] = np.nan
    poisoned = Law(law.tau_ff, q_ref, law.kp, law.kd, law.dq_ref, law.lim)
    fwp = fw[:5] + (_feedback_of(torch, poisoned, "sample", hold),)
    got = _fbp_adjoint(torch, chain, fwp, integrator, **kw)
    assert got["status"][bad] == -1 and (got["status"][others] == 1).all() and np.isfinite(got["gpi"]).all() and np.isfinite(got["gcomp"]).all()
    for k in ("gq0", "gdq0", "gkp", "gkd", "glim"):
        assert np.isnan(got[k][bad]).all() and np.array_equal(got[k][others], clean[k][others]), k
    for k in ("gtau", "gq_ref", "gdq_ref"):
        assert np.isnan(got[k][:2, bad]).all() and np.array_equal(got[k][2, bad], clean[k][2, bad]) and np.array_equal(got[k][:, others], clean[k][:, others]), k
    sub = lambda x: x if x.ndim == 1 else np.ascontiguousarray(x[..., others, :])
    law2 = Law(sub(law.tau_ff), sub(law.q_ref), sub(law.kp), sub(law.kd), sub(law.dq_ref), law.lim)
    fw2, st2, _ = _fb_forward(torch, chain, sub(q0), sub(dq0), law2, integrator, hold, components=cs)
    assert (st2 == 1).all()
    kw2 = dict(gq_end=sub(gq), gdq_end=sub(gv), gq_traj=sub(rq), gdq_traj=sub(rv), components=cs)
    want = _fbp_adjoint(torch, chain, fw2, integrator, **kw2)
    _, api, _, acomp = _expected(torch, chain, cs, law2, sub(q0), sub(dq0), _host_seq(fw2[3], "sample"), _host_seq(fw2[4], "sample"), T, sub(gq),
                                 sub(gv), sub(rq), sub(rv), None, integrator, hold)
    w = max(_within(got["gpi"], want["gpi"], api, 1e-11, "gpi"), _within(got["gcomp"], want["gcomp"], acomp, 1e-11, "gcomp"))
    print("%s %s: with the failed sample against the batch without it, worst distance / sum of absolute rows %.3g (bound 1e-11)"
          % (name, MODE_IDS[MODES.index(mode)], w))


# ---- 5. a captured graph
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_replays_from_a_captured_graph(mode):
    """one call captured on a single stream, every buffer made beforehand, replayed on new seeds"""
    torch = pytest.importorskip("torch")
    integrator, hold = mode
    name = "ur10_like"
    chain = _chain(name)
    n, N, T = chain.getActiveJointsNumber(), 130, 3
    q0, dq0, tau = _inputs(name, n, N, T, seed=14900)
    law = _law(name, n, N, T, 14900, limits=True, q0=q0, dq0=dq0, tau=tau)
    fw, st, _ = _fb_forward(torch, chain, q0, dq0, law, integrator, hold)
    assert (st == 1).all()
    tq, tdq, ttau, q_traj, dq_traj, fb = fw[:6]
    gq, gv = (torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(2))
    gu = torch.rand((T, N, n), dtype=torch.float64, device="cuda") * 2 - 1
    call = lambda: chain.rolloutParameterAdjoint(tq, tdq, ttau, DT, q_traj, dq_traj, gq_end=gq, gDq_end=gv, integrator=integrator, feedback=fb,
                                                 want_feedback=("q_ref", "Dq_ref", "kp", "kd", "tau_limit"), gu_traj=gu)
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
        gu.uniform_(-1, 1)
        g.replay()
        torch.cuda.synchronize()
        again = call()
        assert len(res) == len(again) == 11
        for x, y in zip(res, again):
            assert (x is None and y is None) or torch.equal(x, y)
        assert bool((res[5] == 1).all()) and bool(res[3].abs().sum() > 0)


# ---- 6., 7. central differences of the library's closed-loop rollout over Chain.withParameters
def _library_side(torch, chain, x, seeds, integrator, hold):
    """loss(p) -> (L per sample, the command record) of the library's closed loop on chain.withParameters(p), and the per-sample gpi of the
    nominal model (N, P): rolloutParameterAdjoint(feedback=) on every sample alone (the call returns sums over the samples)"""
    cq, cv, rq, rv, cu = seeds
    N = len(cq)
    law = Law(x["tau"], x["q_ref"], x["kp"], x["kd"], x["dq_ref"], x["lim"])
    tq, tdq, ttau = _dev(torch, x["q0"], "sample"), _dev(torch, x["dq0"], "sample"), _dev_seq(torch, x["tau"], "sample")
    fb = _feedback_of(torch, law, "sample", hold, command_trajectory=True)

    def loss(p):
        r = chain.withParameters(p).rollout(tq, tdq, ttau, DT, integrator=integrator, trajectory_every=1, feedback=fb)
        assert bool((r[2] == 1).all())
        q_traj, v_traj, u = (_host_seq(t, "sample") for t in r[3:6])
        return _loss_terms(seeds, r[0].cpu().numpy(), r[1].cpu().numpy(), q_traj, v_traj, u)[0], u

    fw = chain.rollout(tq, tdq, ttau, DT, integrator=integrator, trajectory_every=1, feedback=fb)
    tcq, tcv = _dev(torch, cq, "sample"), _dev(torch, cv, "sample")
    trq, trv, tcu = (_dev_seq(torch, a, "sample") for a in (rq, rv, cu))
    from rosdyn_amd import Feedback
    gpi = np.empty((N, 10 * chain.getJointsNumber()))
    for s in range(N):
        one = lambda t: t[..., s:s + 1, :].contiguous()
        fb1 = Feedback(one(fb.q_ref), one(fb.kp), one(fb.kd), one(fb.Dq_ref), hold=hold, tau_limit=fb.tau_limit)
        r = chain.rolloutParameterAdjoint(one(tq), one(tdq), one(ttau), DT, one(fw[3]), one(fw[4]), gq_end=one(tcq), gDq_end=one(tcv),
                                          gq_traj=one(trq), gDq_traj=one(trv), integrator=integrator, feedback=fb1, gu_traj=one(tcu))
        assert int(r[5][0]) == 1
        gpi[s] = r[3].cpu().numpy()
    whole = chain.rolloutParameterAdjoint(tq, tdq, ttau, DT, fw[3], fw[4], gq_end=tcq, gDq_end=tcv, gq_traj=trq, gDq_traj=trv, integrator=integrator,
                                          feedback=fb, gu_traj=tcu)[3].cpu().numpy()
    assert (np.abs(whole - gpi.sum(axis=0)) <= 1e-12 * np.abs(gpi).sum(axis=0)).all()
    return loss, gpi


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", CD_CHAINS)
def test_directional_consistency_with_central_differences_without_limits(name, mode):
    """Asserted: err(H) / err(H / 2) in [3.5, 4.5] on the samples with err(H) >= 1e-9 scale, at least three quarters of the batch, and
    err(H) / scale <= 2 x the oracle's worst figure (FBP_ORACLE_WORST)."""
    torch = pytest.importorskip("torch")
    integrator, hold = mode
    chain = _chain(name)
    x, seeds = _case(name, chain.getActiveJointsNumber())
    N = len(seeds[0])
    pi = chain.getNominalParameters()
    delta = _direction(pi)
    loss, gpi = _library_side(torch, chain, x, seeds, integrator, hold)
    lin = gpi @ delta
    scale = np.abs((gpi * delta).reshape(N, -1, 10).sum(axis=2)).max(axis=1)
    errs = [np.abs((loss(pi + h * delta)[0] - loss(pi - h * delta)[0]) / (2.0 * h) - lin) / scale for h in (CD_H, 0.5 * CD_H)]
    sel = errs[0] >= 1e-9
    ratio = errs[0][sel] / errs[1][sel]
    cap = 2.0 * FBP_ORACLE_WORST[(name, integrator, bool(hold))]
    print("%s %s: directional err(H) / scale max %.3g (cap %.3g), err ratio %.4g .. %.4g over %d of %d samples (bounds 3.5, 4.5)"
          % (name, MODE_IDS[MODES.index(mode)], errs[0].max(), cap, ratio.min(), ratio.max(), int(sel.sum()), N))
    assert int(sel.sum()) >= 3 * N // 4 and ratio.min() >= 3.5 and ratio.max() <= 4.5, (int(sel.sum()), float(ratio.min()), float(ratio.max()))
    assert errs[0].max() <= cap, (float(errs[0].max()), cap)


@pytest.mark.parametrize("mode", LIMIT_MODES, ids=["euler", "rk4-hold"])
@pytest.mark.parametrize("name", CD_CHAINS)
def test_directional_consistency_with_central_differences_with_limits(name, mode):
    """Over the samples whose clamp pattern is the same in the unperturbed run and in both perturbed runs -- at least half of the batch --
    |CD(h) - <gpi, delta>| / scale <= 8 x the oracle's own |CD(h) - CD(h / 2)| / scale (FBP_LIMIT_NOISE), h = FBP_LIMIT_STEP."""
    torch = pytest.importorskip("torch")
    integrator, hold = mode
    chain = _chain(name)
    x, seeds = _case(name, chain.getActiveJointsNumber(), limits=True)
    N = len(seeds[0])
    pi = chain.getNominalParameters()
    delta = _direction(pi)
    loss, gpi = _library_side(torch, chain, x, seeds, integrator, hold)
    h = FBP_LIMIT_STEP[name]
    (lp, up), (lm, um), (_, u0) = loss(pi + h * delta), loss(pi - h * delta), loss(pi)
    share = _clamped_share(u0, x["lim"])
    keep = _same_pattern(x["lim"], u0, (up, x["lim"]), (um, x["lim"]))
    scale = np.abs((gpi * delta).reshape(N, -1, 10).sum(axis=2)).max(axis=1)
    err = (np.abs((lp - lm) / (2.0 * h) - gpi @ delta) / scale)[keep]
    bound = 8.0 * FBP_LIMIT_NOISE[(name, integrator)]
    print("%s %s: %.1f %% clamped, %d of %d samples keep their pattern at h = %g, err / scale max %.3g (bound %.3g)"
          % (name, integrator, 100.0 * share, int(keep.sum()), N, h, err.max(), bound))
    assert 0.2 <= share <= 0.8 and 2 * int(keep.sum()) >= N
    assert err.max() <= bound, (float(err.max()), bound)
