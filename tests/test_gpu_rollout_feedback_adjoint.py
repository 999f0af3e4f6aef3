"""GPU tests of rdyn_rollout_adjoint_feedback / Chain.rolloutAdjoint(feedback=) / autograd.rollout(feedback=): the exact transpose of the
closed loop Chain.rollout(feedback=) integrates, with the gradients with respect to references, gains and limits.

1. One step against the library's own product: the numpy closed-loop adjoint of _feedback_adjoint.py runs over getJointAccelerationVjp /
   getJointAcceleration (with and without wrenches and components) and is compared with the call for every output.  Bound per sample
   and entry: 1e-11 x the same composition on magnitudes (test_gpu_rollout_adjoint_ext.py's bound, the law's terms in absolute value).
   With limits a sample is left out when a raw command of the numpy run lies within 1e-9 lim of a limit (at most 1 % may be).
2. Saturation structure, exact: a joint clamped at every evaluation has zero columns but in glim; limits far above every command
   change no bit and give glim == 0.
3. Semi-implicit Euler: hold = 0 and hold = 1 give the same bits.
4. Zero gains give the bits of rolloutAdjoint(ext_wrenches=); fb == NULL through the new entry point gives the base call's bits.
5. A horizon split anywhere into two chained calls (accumulate on the earlier part) gives the single call's bits, gkp / gkd / glim included.
6. Directional consistency against central differences of Chain.rollout(feedback=) along (x0, tau_ff, q_ref, dq_ref, kp, kd, wrench).
   Without limits: the bound is the truncation of the difference itself, measured on the CPU oracle, and err(h) / err(h / 2) is about 4.
   With limits under hold = 1: the samples whose clamp pattern is the same in all three runs, at the step the oracle chose; the limits
   are a direction too (_feedback_adjoint.py has both derivations).
7. autograd: loss.backward() through autograd.rollout(feedback=).
8. Failures, T = 0 and T = 1, aliasing, unsupported chains, a captured graph."""
import ctypes as C

import numpy as np
import pytest

from _arrays import DT, EPS, INTEGRATORS, _dev, _dev_seq, _host, _host_seq, _seeds, _wrench_rollout_inputs as _inputs, _wrenches
from _chains import _chain, _trio
from _components import _set, _specs
from _feedback import Law, _limits, _scale
from _feedback_adjoint import _fb_adjoint, _fb_forward, _feedback_of, _law, _lib_closures, _np_fb_adjoint

pytestmark = pytest.mark.gpu
CHAINS = ["planar_2r", "mixed_joints", "ur10_like", "panda_like", "ur10_public", "ur10_permuted", "rev10"]
LAYOUTS = ("sample", "element")
OUTPUTS = ("gq0", "gdq0", "gtau", "gq_ref", "gdq_ref", "gkp", "gkd", "glim", "gext")
MODES = [("semi_implicit_euler", True), ("rk4", True), ("rk4", False)]
MODE_IDS = ["euler", "rk4-hold", "rk4-continuous"]


def _same(a, b, keys=None):
    keys = keys or [k for k in a if k in b]
    return all(np.array_equal(a[k], b[k]) for k in keys)


# ---- 1. one step against the library's own product
VARIANTS = {
    # per-sample gains, limits, kd, dq_ref, wrenches, components
    "shared": (False, False, True, True, False, False),
    "per_sample_wrenches_components": (True, False, True, True, True, True),
    "limits": (False, True, True, True, False, False),
    "limits_per_sample_wrenches": (True, True, True, True, True, False),
    "no_kd": (False, False, False, False, False, False),
    "no_dq_ref": (False, True, True, False, False, True),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", CHAINS + ["ur10_public_long"])
def test_one_step_against_the_library_own_product(name, mode, variant):
    torch = pytest.importorskip("torch")
    integrator, hold = mode
    per_sample, limits, with_kd, with_dq_ref, wrenches, components = VARIANTS[variant]
    if name == "ur10_public_long":
        wrenches = False   # the reduced companion serves the closed loop without wrenches only
    chain, _, chain0 = _trio(name)
    n, L = chain.getActiveJointsNumber(), chain.getLinksNumber()
    cs = _set(_specs(n), n) if components else None
    worst, left_out, total = 0.0, 0, 0
    for N in (1, 63, 64, 65, 200):
        q0, dq0, tau = _inputs(name, n, N, 1, seed=12100 + N)
        gq, gv, gu, _ = _seeds(n, N, 1, seed=12100 + N)
        law = _law(name, n, N, 1, 12100 + N, per_sample, limits, with_kd, with_dq_ref, q0, dq0, tau)
        W = _wrenches(name, N, L, seed=12150 + N) if wrenches else None
        for link in ((None, L - 1) if wrenches else (None,)):
            Wl = W if (W is None or link is None) else W[:, link]
            fd, vjp, avjp, box = _lib_closures(torch, chain, chain0, cs, Wl, link)
            want = _np_fb_adjoint(vjp, fd, law, q0, dq0, None, None, 1, gq, gv, DT, integrator, hold, gu=gu)
            mag = _np_fb_adjoint(avjp, fd, law, q0, dq0, None, None, 1, gq, gv, DT, integrator, hold, gu=gu, mag=True)
            want["gext"], mag["gext"] = box["g"], box["m"]
            got = None
            for layout in LAYOUTS:
                fw, st, _ = _fb_forward(torch, chain, q0, dq0, law, integrator, hold, layout, W=Wl, link=link, components=cs)
                assert (st == 1).all()
                fw = fw[:3] + (None, None) + fw[5:]
                r = _fb_adjoint(torch, chain, fw, integrator, layout, gq_end=gq, gdq_end=gv, gu=gu, components=cs)
                assert r["status"].shape == (N,) and (r["status"] == 1).all()
                if got is not None:
                    assert _same(got, r), "the layouts give the same bits"
                got = r
            keep = ~want["near"]
            left_out, total = left_out + int((~keep).sum()), total + N
            for what in OUTPUTS:
                if what not in got:
                    continue
                g, w, m = got[what], want[what], mag[what]
                g = g[0] if what in ("gtau", "gq_ref", "gdq_ref", "gext") else g
                w = w[0] if what in ("gtau", "gq_ref", "gdq_ref") else w
                m = m[0] if what in ("gtau", "gq_ref", "gdq_ref") else m
                g, w, m = g[keep], w[keep], m[keep]
                assert np.isfinite(g).all() and g.shape == w.shape, what
                assert (g[m == 0] == 0.0).all() and (w[m == 0] == 0.0).all(), what   # nothing enters the entry on either side
                sel = m > 0
                if sel.any():
                    ratio = float((np.abs(g - w)[sel] / m[sel]).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1e-11, (what, N, link, ratio)
    print("%s %s %s: worst distance / sum of absolute terms %.3g (bound 1e-11), %d of %d samples left out" % (name, MODE_IDS[MODES.index(mode)],
                                                                                                             variant, worst, left_out, total))
    assert left_out <= 0.01 * total


# ---- 2. saturation structure, exact
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["planar_2r", "ur10_like", "rev10"])
def test_saturation_structure_is_exact(name, mode):
    torch = pytest.importorskip("torch")
    integrator, hold = mode
    chain = _chain(name)
    n, N, T = chain.getActiveJointsNumber(), 65, 4
    q0, dq0, tau = _inputs(name, n, N, T, seed=12300)
    gq, gv, rq, rv = _seeds(n, N, T, seed=12300)
    gu = _seeds(n, N, T, seed=12320)[2]
    base = _law(name, n, N, T, 12300, q0=q0, dq0=dq0, tau=tau)
    kw = dict(gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, gu=gu)
    # joint j clamped at every evaluation: its limit far below every command, and a feed-forward term that keeps the command off zero
    j = n - 1
    lim = 1e30 * np.ones(n)
    lim[j] = 1e-6 * _scale(name)
    ff = tau.copy()
    ff[:, :, j] = 50.0 * _scale(name) * np.where(ff[:, :, j] >= 0, 1.0, -1.0)
    law = Law(ff, base.q_ref, base.kp, base.kd, base.dq_ref, lim)
    fw, st, u = _fb_forward(torch, chain, q0, dq0, law, integrator, hold)
    assert (st == 1).all() and (np.abs(u[:, :, j]) == lim[j]).all()
    r = _fb_adjoint(torch, chain, fw, integrator, **kw)
    assert (r["status"] == 1).all()
    for what in ("gtau", "gq_ref", "gdq_ref", "gkp", "gkd"):
        assert (r[what][..., j] == 0.0).all(), what
        assert np.abs(np.delete(r[what], j, axis=-1)).min() > 0, what
    assert (r["glim"][:, j] != 0.0).all() and (np.delete(r["glim"], j, axis=1) == 0.0).all()
    # limits far above every command: the bits of the call without limits, and glim == 0
    far = Law(tau, base.q_ref, base.kp, base.kd, base.dq_ref, 1e30 * np.ones(n))
    a = _fb_adjoint(torch, chain, _fb_forward(torch, chain, q0, dq0, far, integrator, hold)[0], integrator, **kw)
    b = _fb_adjoint(torch, chain, _fb_forward(torch, chain, q0, dq0, base, integrator, hold)[0], integrator, **kw)
    assert (a["glim"] == 0.0).all() and "glim" not in b
    assert _same(a, b, [k for k in b]) and all(np.isfinite(b[k]).all() for k in b)


# ---- 3. semi-implicit Euler: one computation under both modes
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["mixed_joints", "panda_like", "ur10_public_long"])
def test_euler_gives_the_same_bits_under_both_hold_modes(name, layout):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, L, N, T = chain.getActiveJointsNumber(), chain.getLinksNumber(), 65, 4
    q0, dq0, tau = _inputs(name, n, N, T, seed=12400)
    gq, gv, rq, rv = _seeds(n, N, T, seed=12400)
    law = _law(name, n, N, T, 12400, per_sample=True, limits=True, q0=q0, dq0=dq0, tau=tau)
    W = None if name == "ur10_public_long" else _wrenches(name, N, L, seed=12450)
    res = []
    for hold in (True, False):
        fw, st, _ = _fb_forward(torch, chain, q0, dq0, law, "semi_implicit_euler", hold, layout, W=W)
        assert (st == 1).all()
        res.append(_fb_adjoint(torch, chain, fw, "semi_implicit_euler", layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, gu=rq))
    assert _same(res[0], res[1], list(res[0])) and np.abs(res[0]["glim"]).max() > 0 and np.abs(res[0]["gkd"]).max() > 0


# ---- 4. zero gains: the open loop's bits; fb == NULL: the base call
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["ur10_like", "rev10"])
def test_zero_gains_give_the_bits_of_the_open_loop(name, mode):
    torch = pytest.importorskip("torch")
    from rosdyn_amd._lib import INTEGRATORS as CODES, Batch, ExtWrenches, ExtWrenchGradient, FeedbackGradient, RolloutAdjointDesc, check, lib
    integrator, hold = mode
    chain = _chain(name)
    n, L, N, T = chain.getActiveJointsNumber(), chain.getLinksNumber(), 65, 4
    q0, dq0, tau = _inputs(name, n, N, T, seed=12500)
    gq, gv, rq, rv = _seeds(n, N, T, seed=12500)
    base = _law(name, n, N, T, 12500, q0=q0, dq0=dq0, tau=tau)
    law = Law(tau, base.q_ref, np.zeros(n), np.zeros(n), base.dq_ref)
    W = _wrenches(name, N, L, seed=12550)
    fw, st, _ = _fb_forward(torch, chain, q0, dq0, law, integrator, hold, W=W)
    assert (st == 1).all()
    r = _fb_adjoint(torch, chain, fw, integrator, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv)
    tq, tdq, ttau, q_traj, dq_traj, _, tw, _ = fw
    d = lambda x: _dev_seq(torch, x, "sample") if x.ndim == 3 else _dev(torch, x, "sample")
    open_fw = chain.rollout(tq, tdq, ttau, DT, integrator=integrator, trajectory_every=1, ext_wrenches=tw)
    assert torch.equal(open_fw[3], q_traj) and torch.equal(open_fw[4], dq_traj)
    o = chain.rolloutAdjoint(tq, tdq, ttau, DT, q_traj, dq_traj, gq_end=d(gq), gDq_end=d(gv), gq_traj=d(rq), gDq_traj=d(rv), integrator=integrator,
                             ext_wrenches=tw, want_ext=True)
    assert np.array_equal(r["gq0"], o[0].cpu().numpy()) and np.array_equal(r["gdq0"], o[1].cpu().numpy())
    assert np.array_equal(r["gtau"], o[2].cpu().numpy()) and np.array_equal(r["gext"], o[4].cpu().numpy())
    assert (r["gq_ref"] == 0.0).all() and (r["gdq_ref"] == 0.0).all() and (r["status"] == 1).all()
    # fb == NULL through the new entry point: the base call's bits, and a feedback gradient is an argument error
    gq0, gdq0, gtau, gw = torch.full_like(tq, 7.0), torch.full_like(tq, 7.0), torch.full_like(ttau, 7.0), torch.full((T, N, L, 6), 7.0, dtype=torch.float64, device="cuda")
    status = torch.zeros((N,), dtype=torch.int32, device="cuda")
    tgq, tgv, trq, trv = d(gq), d(gv), d(rq), d(rv)
    ds = RolloutAdjointDesc()
    ds.n_steps, ds.integrator, ds.dt = T, CODES[integrator], DT
    ds.tau, ds.tau_step_stride = ttau.data_ptr(), n * N
    ds.q_traj, ds.dq_traj, ds.traj_step_stride = q_traj.data_ptr(), dq_traj.data_ptr(), n * N
    ds.gq_end, ds.gdq_end, ds.gq_traj, ds.gdq_traj, ds.gtraj_step_stride = tgq.data_ptr(), tgv.data_ptr(), trq.data_ptr(), trv.data_ptr(), n * N
    ds.gq0, ds.gdq0, ds.gtau, ds.gtau_step_stride, ds.status = gq0.data_ptr(), gdq0.data_ptr(), gtau.data_ptr(), n * N, status.data_ptr()
    x, g = ExtWrenches(), ExtWrenchGradient()
    x.w, x.link, x.step_stride = tw.data_ptr(), -1, 0
    g.gw, g.step_stride = gw.data_ptr(), 6 * L * N
    b = Batch()
    b.n_samples, b.q, b.dq, b.ddq, b.layout, b.device = N, tq.data_ptr(), tdq.data_ptr(), None, 0, -1
    b.stream = torch.cuda.current_stream().cuda_stream
    check(lib().rdyn_rollout_adjoint_feedback(chain._h, C.byref(b), C.byref(ds), None, 0, C.byref(x), C.byref(g), None, None, 0, None, 0))
    assert torch.equal(gq0, o[0]) and torch.equal(gdq0, o[1]) and torch.equal(gtau, o[2]) and torch.equal(status, o[3]) and torch.equal(gw, o[4])
    gf = FeedbackGradient()
    gf.gkp = gq0.data_ptr()
    assert lib().rdyn_rollout_adjoint_feedback(chain._h, C.byref(b), C.byref(ds), None, 0, C.byref(x), C.byref(g), None, C.byref(gf), 0, None, 0) == 1


# ---- 5. the horizon can be split anywhere, bitwise
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", MODES + [("semi_implicit_euler", False)], ids=MODE_IDS + ["euler-continuous"])
@pytest.mark.parametrize("name", ["mixed_joints", "ur10_public", "rev10"])
def test_the_horizon_can_be_split_anywhere_bitwise(name, mode, layout):
    torch = pytest.importorskip("torch")
    integrator, hold = mode
    chain = _chain(name)
    n, L, N, T = chain.getActiveJointsNumber(), chain.getLinksNumber(), 65, 5
    cs = _set(_specs(n), n)
    q0, dq0, tau = _inputs(name, n, N, T, seed=12600)
    gq, gv, rq, rv = _seeds(n, N, T, seed=12600)
    gu = _seeds(n, N, T, seed=12620)[3]
    law = _law(name, n, N, T, 12600, per_sample=True, limits=True, q0=q0, dq0=dq0, tau=tau)
    W = np.array([_wrenches(name, N, L, seed=12650 + t) for t in range(T)])
    fw, st, _ = _fb_forward(torch, chain, q0, dq0, law, integrator, hold, layout, W=W, wseq=True, components=cs)
    assert (st == 1).all()
    tq, tdq, ttau, q_traj, dq_traj, fb, tw, _ = fw
    whole = _fb_adjoint(torch, chain, fw, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, gu=gu, components=cs)
    assert (whole["status"] == 1).all() and all(np.isfinite(whole[k]).all() and np.abs(whole[k]).max() > 0 for k in OUTPUTS)
    seq = ("gtau", "gq_ref", "gdq_ref", "gext")
    shape = tuple(tq.shape)
    for cut in range(1, T):
        sums = {k: torch.full(shape, 5.0, dtype=torch.float64, device="cuda") for k in ("gkp", "gkd", "gtau_limit")}
        later_law = Law(law.tau_ff[cut:], law.q_ref[cut:], law.kp, law.kd, law.dq_ref[cut:], law.lim)
        later = (q_traj[cut - 1], dq_traj[cut - 1], ttau[cut:], q_traj[cut:], dq_traj[cut:], _feedback_of(torch, later_law, layout, hold), tw[cut:], None)
        b = _fb_adjoint(torch, chain, later, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq[cut:], gdq_traj=rv[cut:], gu=gu[cut:],
                        components=cs, out=dict(sums))
        earlier_law = Law(law.tau_ff[:cut], law.q_ref[:cut], law.kp, law.kd, law.dq_ref[:cut], law.lim)
        earlier = (tq, tdq, ttau[:cut], q_traj[:cut], dq_traj[:cut], _feedback_of(torch, earlier_law, layout, hold), tw[:cut], None)
        a = _fb_adjoint(torch, chain, earlier, integrator, layout, gq_end=b["gq0"], gdq_end=b["gdq0"], gq_traj=rq[:cut], gdq_traj=rv[:cut],
                        gu=gu[:cut], components=cs, out=dict(sums), accumulate=True)
        assert (a["status"] == 1).all() and (b["status"] == 1).all()
        assert _same(a, whole, ("gq0", "gdq0", "gkp", "gkd", "glim")), cut
        assert all(np.array_equal(np.concatenate([a[k], b[k]]), whole[k]) for k in seq), cut
    # the summed reference gradient (one record) against the per-step records, to rounding: T additions on either side
    tot = _fb_adjoint(torch, chain, fw, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, gu=gu, components=cs, sum_ref=True)
    assert _same(tot, whole, ("gq0", "gdq0", "gtau", "gkp", "gkd", "glim", "gext"))
    for k in ("gq_ref", "gdq_ref"):
        assert tot[k].shape == (N, n)
        exact = whole[k].astype(np.longdouble).sum(axis=0)
        assert (np.abs(tot[k] - exact) <= T * EPS * np.abs(whole[k]).sum(axis=0)).all(), k


# ---- 7. autograd
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["ur10_like", "ur10_public"])
def test_backward_through_the_closed_loop(name, mode):
    torch = pytest.importorskip("torch")
    from rosdyn_amd import Feedback, autograd
    integrator, hold = mode
    chain = _chain(name)
    n, L, N, T = chain.getActiveJointsNumber(), chain.getLinksNumber(), 5, 4
    q0, dq0, tau = _inputs(name, n, N, T, seed=12700)
    cq, cv, ct, _ = _seeds(n, N, T, seed=12700)
    law = _law(name, n, N, T, 12700, limits=True, q0=q0, dq0=dq0, tau=tau)
    leaf = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda().requires_grad_(True)
    tq, tdq, ttau, q_ref, dq_ref, kp, kd, lim, w = (leaf(x) for x in (q0, dq0, tau, law.q_ref, law.dq_ref, law.kp, law.kd, law.lim,
                                                                     _wrenches(name, N, L, seed=12750)))
    tcq, tcv, tct = (torch.from_numpy(x).cuda() for x in (cq, cv, ct))
    fb = Feedback(q_ref, kp, kd, dq_ref, hold=hold, tau_limit=lim, command_trajectory=True)
    q_end, dq_end, q_traj, dq_traj, u = autograd.rollout(chain, tq, tdq, ttau, DT, integrator=integrator, trajectory=True, ext_wrenches=w,
                                                         feedback=fb)
    ((tcq * q_end).sum() + (tcv * dq_end).sum() + (tct * q_traj).sum() + (tct * u).sum()).backward()
    leaves = dict(q0=tq, dq0=tdq, tau=ttau, q_ref=q_ref, dq_ref=dq_ref, kp=kp, kd=kd, lim=lim, w=w)
    assert all(t.grad is not None and tuple(t.grad.shape) == tuple(t.shape) and bool(torch.isfinite(t.grad).all()) and bool(t.grad.abs().sum() > 0)
               for t in leaves.values())
    # the direct call: the same bits, shared gains and limits as the sums of the per-sample rows, the held wrench as the sum over the steps
    det = lambda t: t.detach()
    fbd = Feedback(det(q_ref), det(kp), det(kd), det(dq_ref), hold=hold, tau_limit=det(lim), command_trajectory=True)
    r = chain.rollout(det(tq), det(tdq), det(ttau), DT, integrator=integrator, trajectory_every=1, ext_wrenches=det(w), feedback=fbd)
    assert torch.equal(r[5], u.detach())
    a = chain.rolloutAdjoint(det(tq), det(tdq), det(ttau), DT, r[3], r[4], gq_end=tcq, gDq_end=tcv, gq_traj=tct, integrator=integrator,
                             ext_wrenches=det(w), want_ext=True, sum_ext=True, feedback=fbd,
                             want_feedback=("q_ref", "Dq_ref", "kp", "kd", "tau_limit"), gu_traj=tct)
    for t, g in zip((tq, tdq, ttau, w, q_ref, dq_ref), a[:3] + a[4:7]):
        assert torch.equal(t.grad, g)
    for t, rows in zip((kp, kd, lim), a[7:]):
        assert tuple(rows.shape) == (N, n) and torch.equal(t.grad, rows.sum(dim=0))
    # a held reference and per-sample gains
    q_ref1, kp1, kd1 = leaf(law.q_ref[0]), leaf(np.tile(law.kp, (N, 1))), leaf(np.tile(law.kd, (N, 1)))
    fb1 = Feedback(q_ref1, kp1, kd1, None, hold=hold)
    q_end, dq_end = autograd.rollout(chain, det(tq), det(tdq), det(ttau), DT, integrator=integrator, feedback=fb1)
    ((tcq * q_end).sum() + (tcv * dq_end).sum()).backward()
    r = chain.rollout(det(tq), det(tdq), det(ttau), DT, integrator=integrator, trajectory_every=1, feedback=Feedback(det(q_ref1), det(kp1), det(kd1), hold=hold))
    per = chain.rolloutAdjoint(det(tq), det(tdq), det(ttau), DT, r[3], r[4], gq_end=tcq, gDq_end=tcv, integrator=integrator,
                               feedback=Feedback(det(q_ref1), det(kp1), det(kd1), hold=hold), want_feedback=("q_ref", "kp", "kd"), sum_ref=False)
    assert tuple(q_ref1.grad.shape) == (N, n) and tuple(per[4].shape) == (T, N, n)
    assert bool(((q_ref1.grad - per[4].sum(dim=0)).abs() <= T * EPS * per[4].abs().sum(dim=0)).all())
    assert torch.equal(kp1.grad, per[5]) and torch.equal(kd1.grad, per[6])
    with pytest.raises(ValueError, match="follow-up"):
        autograd.rollout(chain, det(tq), det(tdq), det(ttau), DT, feedback=fb1, parameters=torch.zeros(10 * chain.getJointsNumber(), dtype=torch.float64))


# ---- 8. failures, boundaries, capture
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["ur10_like", "rev10"])
def test_a_failed_sample_is_nan_in_its_own_outputs_only(name, mode):
    torch = pytest.importorskip("torch")
    integrator, hold = mode
    chain = _chain(name)
    n, N, T = chain.getActiveJointsNumber(), 130, 4
    q0, dq0, tau = _inputs(name, n, N, T, seed=12800)
    gq, gv, rq, rv = _seeds(n, N, T, seed=12800)
    law = _law(name, n, N, T, 12800, per_sample=True, limits=True, q0=q0, dq0=dq0, tau=tau)
    kw = dict(gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, gu=rv)
    fw, st, _ = _fb_forward(torch, chain, q0, dq0, law, integrator, hold)
    clean = _fb_adjoint(torch, chain, fw, integrator, **kw)
    assert (st == 1).all() and (clean["status"] == 1).all()
    bad, others = 66, np.arange(N) != 66
    rows, seqs = ("gq0", "gdq0", "gkp", "gkd", "glim"), ("gtau", "gq_ref", "gdq_ref")

    def check(got, from_step=T):
        assert got["status"][bad] == -1 and (got["status"][others] == 1).all()
        assert all(np.isnan(got[k][bad]).all() for k in rows) and all(np.isnan(got[k][:from_step, bad]).all() for k in seqs)
        assert all(np.array_equal(got[k][from_step:, bad], clean[k][from_step:, bad]) for k in seqs)
        assert all(np.array_equal(got[k][others], clean[k][others]) for k in rows)
        assert all(np.array_equal(got[k][:, others], clean[k][:, others]) for k in seqs)

    tq, tdq, ttau, q_traj, dq_traj, fb, tw, lname = fw
    # NaN in a reference of step 1, in a gain of the sample: from the backward step that reads it on
    from rosdyn_amd import Feedback
    q_ref = fb.q_ref.clone()
    q_ref[1, bad, 0] = float("nan")
    check(_fb_adjoint(torch, chain, fw[:5] + (Feedback(q_ref, fb.kp, fb.kd, fb.Dq_ref, hold=hold, tau_limit=fb.tau_limit),) + fw[6:], integrator, **kw), 2)
    kd = fb.kd.clone()
    kd[bad, n - 1] = float("inf")
    check(_fb_adjoint(torch, chain, fw[:5] + (Feedback(fb.q_ref, fb.kp, kd, fb.Dq_ref, hold=hold, tau_limit=fb.tau_limit),) + fw[6:], integrator, **kw))
    # a sample whose forward rollout failed
    q0b = q0.copy()
    q0b[bad, 0] = np.nan
    fwb, stb, _ = _fb_forward(torch, chain, q0b, dq0, law, integrator, hold)
    assert stb[bad] == -1 and (stb[others] == 1).all()
    check(_fb_adjoint(torch, chain, fwb, integrator, **kw))
    # a NaN limit fails every sample (the limits are shared)
    lim = fb.tau_limit.clone()
    lim[0] = float("nan")
    got = _fb_adjoint(torch, chain, fw[:5] + (Feedback(fb.q_ref, fb.kp, fb.kd, fb.Dq_ref, hold=hold, tau_limit=lim),) + fw[6:], integrator, **kw)
    assert (got["status"] == -1).all() and all(np.isnan(got[k]).all() for k in rows + seqs)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["panda_like", "ur10_public_long"])
def test_no_steps_one_step_and_aliasing(name, mode):
    torch = pytest.importorskip("torch")
    integrator, hold = mode
    chain = _chain(name)
    n, N, T = chain.getActiveJointsNumber(), 65, 3
    q0, dq0, tau = _inputs(name, n, N, T, seed=12900)
    gq, gv, rq, rv = _seeds(n, N, T, seed=12900)
    law = _law(name, n, N, T, 12900, limits=True, q0=q0, dq0=dq0, tau=tau)
    for layout in LAYOUTS:
        fw, st, _ = _fb_forward(torch, chain, q0, dq0, law, integrator, hold, layout)
        assert (st == 1).all()
        tq, tdq, ttau, q_traj, dq_traj, fb, _, _ = fw
        shape = tuple(tq.shape)
        # T = 0 copies the seeds; the sums are zeros, or left as they are with accumulate
        none = (tq, tdq, ttau[:0], None, None, fb, None, None)
        sums = {k: torch.full(shape, 5.0, dtype=torch.float64, device="cuda") for k in ("gkp", "gkd", "gtau_limit")}
        z = _fb_adjoint(torch, chain, none, integrator, layout, gq_end=gq, gdq_end=gv, out=dict(sums))
        assert np.array_equal(z["gq0"], gq) and np.array_equal(z["gdq0"], gv) and z["gtau"].shape == (0, N, n) and z["gq_ref"].shape == (0, N, n)
        assert all((z[k] == 0.0).all() for k in ("gkp", "gkd", "glim")) and (z["status"] == 1).all()
        for t in sums.values():
            t.fill_(5.0)
        z = _fb_adjoint(torch, chain, none, integrator, layout, gq_end=gq, gdq_end=gv, out=dict(sums), accumulate=True)
        assert np.array_equal(z["gq0"], gq) and all((z[k] == 5.0).all() for k in ("gkp", "gkd", "glim"))
        # T = 1 reads no trajectory: the first step of the split horizon
        per = _fb_adjoint(torch, chain, fw, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv)
        one_law = Law(law.tau_ff[:1], law.q_ref[:1], law.kp, law.kd, law.dq_ref[:1], law.lim)
        one = (tq, tdq, ttau[:1], None, None, _feedback_of(torch, one_law, layout, hold), None, None)
        r1 = _fb_adjoint(torch, chain, one, integrator, layout, gq_end=gq, gdq_end=gv)
        assert (r1["status"] == 1).all() and r1["gtau"].shape == (1, N, n) and all(np.isfinite(r1[k]).all() for k in r1)
        # gq0 / gdq0 written over the end seeds: the same bits
        d = lambda x: _dev_seq(torch, x, layout) if x.ndim == 3 else _dev(torch, x, layout)
        tgq, tgv = d(gq), d(gv)
        r = chain.rolloutAdjoint(tq, tdq, ttau, DT, q_traj, dq_traj, gq_end=tgq, gDq_end=tgv, gq_traj=d(rq), gDq_traj=d(rv), integrator=integrator,
                                 layout=layout, out={"gq0": tgq, "gDq0": tgv}, feedback=fb, want_feedback=("kp", "tau_limit"))
        assert r[0].data_ptr() == tgq.data_ptr() and r[1].data_ptr() == tgv.data_ptr() and len(r) == 6
        assert np.array_equal(_host(r[0], layout), per["gq0"]) and np.array_equal(_host(r[1], layout), per["gdq0"])
        assert np.array_equal(_host_seq(r[2], layout), per["gtau"]) and np.array_equal(_host(r[4], layout), per["gkp"])
        assert np.array_equal(_host(r[5], layout), per["glim"])


@pytest.mark.parametrize("name", ["rev14", "gen20_permuted", "ur10_public_long"])
def test_chains_on_the_chunked_route_are_unsupported(name):
    torch = pytest.importorskip("torch")
    from rosdyn_amd._lib import RdynError
    chain = _chain(name)
    n, L, N, T = chain.getActiveJointsNumber(), chain.getLinksNumber(), 65, 2
    q0, dq0, tau = _inputs(name, n, N, T, seed=13000)
    gq, gv, _, _ = _seeds(n, N, T, seed=13000)
    law = _law(name, n, N, T, 13000, q0=q0, dq0=dq0, tau=tau)
    W = _wrenches(name, N, L, seed=13001)
    for integrator, hold in MODES:
        for with_w in ((True,) if name == "ur10_public_long" else (False, True)):
            fw, st, _ = _fb_forward(torch, chain, q0, dq0, law, integrator, hold, W=W if with_w else None)   # the forward call serves them
            assert (st == 1).all()
            with pytest.raises(RdynError, match="not served yet") as err:
                _fb_adjoint(torch, chain, fw, integrator, gq_end=gq, gdq_end=gv)
            assert err.value.status == 5 and "chunked route" in err.value.message


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["ur10_like", "rev10"])
def test_replays_from_a_captured_graph(name, mode):
    """one adjoint call captured on a single stream (no side branches), replayed on new seeds"""
    torch = pytest.importorskip("torch")
    integrator, hold = mode
    chain = _chain(name)
    n, L, N, T = chain.getActiveJointsNumber(), chain.getLinksNumber(), 200, 4
    q0, dq0, tau = _inputs(name, n, N, T, seed=13100)
    law = _law(name, n, N, T, 13100, per_sample=True, limits=True, q0=q0, dq0=dq0, tau=tau)
    W = np.array([_wrenches(name, N, L, seed=13150 + t) for t in range(T)])
    fw, st, _ = _fb_forward(torch, chain, q0, dq0, law, integrator, hold, W=W, wseq=True)
    tq, tdq, ttau, q_traj, dq_traj, fb, tw, _ = fw
    gq, gv = (torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(2))
    gu = torch.rand((T, N, n), dtype=torch.float64, device="cuda") * 2 - 1
    out = {k: torch.zeros((N, n), dtype=torch.float64, device="cuda") for k in ("gq0", "gDq0", "gkp", "gkd", "gtau_limit")}
    out.update({k: torch.zeros((T, N, n), dtype=torch.float64, device="cuda") for k in ("gtau", "gq_ref", "gDq_ref")})
    out["gext"] = torch.zeros_like(tw)
    want = ("q_ref", "Dq_ref", "kp", "kd", "tau_limit")

    def call():
        return chain.rolloutAdjoint(tq, tdq, ttau, DT, q_traj, dq_traj, gq_end=gq, gDq_end=gv, integrator=integrator, ext_wrenches=tw, want_ext=True,
                                    feedback=fb, want_feedback=want, gu_traj=gu, out=out)

    call()   # first use outside capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            status = call()[3]
    for _ in range(2):
        gq.uniform_(-1, 1)
        gu.uniform_(-1, 1)
        for t in out.values():
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = {k: t.clone() for k, t in out.items()}
        got_status = status.clone()
        again = chain.rolloutAdjoint(tq, tdq, ttau, DT, q_traj, dq_traj, gq_end=gq, gDq_end=gv, integrator=integrator, ext_wrenches=tw, want_ext=True,
                                     feedback=fb, want_feedback=want, gu_traj=gu)
        keys = ("gq0", "gDq0", "gtau", None, "gext", "gq_ref", "gDq_ref", "gkp", "gkd", "gtau_limit")
        assert all(torch.equal(got[k], t) for k, t in zip(keys, again) if k) and torch.equal(got_status, again[3])
        assert bool((got_status == 1).all()) and all(bool(t.abs().sum() > 0) for t in got.values())


# ---- 6. directional consistency against central differences of the closed loop itself
def _directional_forward(torch, chain, seeds, integrator, hold, y):
    """(the forward call's tensors, L, the sum of the absolute terms of L, the command record) at the inputs y"""
    from _feedback_adjoint import _loss_terms
    law = Law(y["tau"], y["q_ref"], y["kp"], y["kd"], y["dq_ref"], y["lim"])
    fw, st, u = _fb_forward(torch, chain, y["q0"], y["dq0"], law, integrator, hold, W=y["W"])
    assert (st == 1).all()
    return (fw,) + _loss_terms(seeds, _host(fw[3][-1], "sample"), _host(fw[4][-1], "sample"), _host_seq(fw[3], "sample"), _host_seq(fw[4], "sample"), u) + (u,)


def _directional_gradient(torch, chain, fw, seeds, integrator, d, limits):
    """{direction: <gradient, direction> per sample} from ONE adjoint call"""
    cq, cv, rq, rv, cu = seeds
    want = ("q_ref", "Dq_ref", "kp", "kd") + (("tau_limit",) if limits else ())
    g = _fb_adjoint(torch, chain, fw, integrator, gq_end=cq, gdq_end=cv, gq_traj=rq, gdq_traj=rv, gu=cu, want=want, sum_ext=True)
    assert (g["status"] == 1).all()
    N = len(cq)
    grads = {"tau": g["gtau"], "q_ref": g["gq_ref"], "dq_ref": g["gdq_ref"], "kp": g["gkp"], "kd": g["gkd"], "wrench": g["gext"]}
    if limits:
        grads["lim"] = g["glim"]   # rows per sample: the sample's own loss against the shared limits
    lin = {"x0": (g["gq0"] * d["x0"][0]).sum(axis=1) + (g["gdq0"] * d["x0"][1]).sum(axis=1)}
    for what, grad in grads.items():
        prod = grad * d[what]
        lin[what] = (np.moveaxis(prod, 0, 1) if prod.ndim == 3 and prod.shape[0] != N else prod).reshape(N, -1).sum(axis=1)
    return lin


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["planar_2r", "mixed_joints", "ur10_like", "panda_like", "ur10_public", "rev10"])
def test_directional_consistency_with_central_differences_of_the_closed_loop(name, mode):
    """Without limits.  Asserted per direction (x0, tau_ff, q_ref, dq_ref, kp, kd, wrench), with err = |central difference - <gradient,
    direction>| / scale: err(h) <= twice the truncation figure the oracle's closed loop alone shows for the chain, mode and direction,
    plus the rounding of the difference quotient; err(h / 2) <= a quarter of that truncation allowance plus its own rounding; and on
    the samples whose err(h) stands clear of the rounding (1000 times it) and of cancellation (a hundredth of the table's figure) the
    ratio err(h) / err(h / 2) lies in [3.5, 4.5]: what is left is the truncation of the difference, not an error of the gradient
    (_feedback_adjoint.py has the derivation and the table).  The loss is linear in the end state, the trajectory records and the
    command record, so gu_traj is exercised."""
    torch = pytest.importorskip("torch")
    from _feedback_adjoint import DIRECTIONAL_H, FB_DIRECTIONAL, FB_DIRECTIONS, _directional_bound, _directional_case, _moved
    integrator, hold = mode
    chain = _chain(name)
    n, L = chain.getActiveJointsNumber(), chain.getLinksNumber()
    x, seeds, d = _directional_case(name, n, L)
    forward = lambda y: _directional_forward(torch, chain, seeds, integrator, hold, y)
    fw, _, scale, _ = forward(x)
    lin = _directional_gradient(torch, chain, fw, seeds, integrator, d, False)
    for what in FB_DIRECTIONS:
        h = DIRECTIONAL_H[what]
        err = [np.abs((forward(_moved(x, d, what, s))[1] - forward(_moved(x, d, what, -s))[1]) / (2.0 * s) - lin[what]) / scale for s in (h, 0.5 * h)]
        bound, half = _directional_bound(name, integrator, hold, what), _directional_bound(name, integrator, hold, what, halved=True)
        clear = err[0] >= max(1000.0 * 64.0 * EPS / h, 0.01 * FB_DIRECTIONAL[(name, integrator, bool(hold))][what])
        ratio = err[0][clear] / err[1][clear]
        print("%s %s %s: directional err / scale %.3g (bound %.3g), at h / 2 %.3g (bound %.3g), ratio %s over %d samples"
              % (name, MODE_IDS[MODES.index(mode)], what, err[0].max(), bound, err[1].max(), half,
                 "%.4g .. %.4g" % (ratio.min(), ratio.max()) if clear.any() else "-", int(clear.sum())))
        assert err[0].max() <= bound and err[1].max() <= half, (what, float(err[0].max()), bound, float(err[1].max()), half)
        assert not clear.any() or (ratio.min() >= 3.5 and ratio.max() <= 4.5), (what, float(ratio.min()), float(ratio.max()))


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", ["planar_2r", "mixed_joints", "ur10_like", "panda_like", "ur10_public", "rev10"])
def test_directional_consistency_with_limits_under_a_held_command(name, integrator):
    """With limits, hold = 1: the command record shows every mask.  Per direction (the seven above and the limits themselves) only the
    samples are kept whose clamp pattern is identical in the unperturbed run and in both perturbed runs; the step is the one the oracle
    alone chose for the chain (FB_LIMIT_STEP); at least half of the samples remain, and on them |central difference - <gradient,
    direction>| / scale <= 8 times the error of the quotient the oracle alone shows (FB_LIMIT_NOISE; _feedback_adjoint.py has the
    derivation).  This checks the clamp's transpose -- the mask and glim -- against a derivative of the forward call."""
    torch = pytest.importorskip("torch")
    from _feedback_adjoint import (FB_LIMIT_NOISE, FB_LIMIT_STEP, LIMIT_DIRECTIONS, _directional_case, _moved_lim, _pattern, _same_pattern)
    chain = _chain(name)
    n, L = chain.getActiveJointsNumber(), chain.getLinksNumber()
    x, seeds, d = _directional_case(name, n, L, limits=True)
    forward = lambda y: _directional_forward(torch, chain, seeds, integrator, True, y)
    fw, _, scale, u0 = forward(x)
    clamped = float((_pattern(u0, x["lim"]) != 0).mean())
    assert 0.2 <= clamped <= 0.8, clamped   # the test is about the clamp
    lin = _directional_gradient(torch, chain, fw, seeds, integrator, d, True)
    h, bound = FB_LIMIT_STEP[name], 8.0 * FB_LIMIT_NOISE[(name, integrator)]
    for what in LIMIT_DIRECTIONS:
        plus, minus = _moved_lim(x, d, what, h), _moved_lim(x, d, what, -h)
        rp, rm = forward(plus), forward(minus)
        keep = _same_pattern(x["lim"], u0, (rp[3], plus["lim"]), (rm[3], minus["lim"]))
        err = (np.abs((rp[1] - rm[1]) / (2.0 * h) - lin[what]) / scale)[keep]
        print("%s %s %s: %d of %d samples keep their clamp pattern (%.0f %% of the commands clamped), directional err / scale %.3g (bound %.3g)"
              % (name, integrator, what, int(keep.sum()), len(keep), 100.0 * clamped, err.max(), bound))
        assert 2 * int(keep.sum()) >= len(keep), (what, int(keep.sum()))
        assert err.max() <= bound, (what, float(err.max()), bound)
