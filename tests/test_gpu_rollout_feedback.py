"""GPU tests of the closed-loop rollouts, rdyn_rollout_feedback / Chain.rollout(feedback=): T steps over
    u = clamp(tau_ff + kp (q_ref - q) + kd (Dq_ref - Dq)),   ddq = FD_E(q, Dq, u, ext_t),
the command held over a step (hold) or formed at every integrator stage.  Checked against (1) the library's own getJointAcceleration at
the stage states, one step, (2) the CPU oracle run through the same law and integrators in numpy, (3) the same with actuator limits that
clamp a fair share of the commands, (4) the command record against the law recomputed from the state records, (5) itself, bitwise: the two
modes under semi-implicit Euler, chained calls, constant set points, repeated gains, chunk sizes, the call without feedback, a captured
graph, (6) the status rule for a NaN reference or gain.  Bounds hold per sample; no sample is excused.
The inputs, the law in numpy and the table of measured bounds (FB_MULTI_STEP: 8 times the oracle's own deviation under a 1e-11 relative
perturbation of every ddq) are tests/_feedback.py's; tests/test_rollout_feedback_inputs.py pins their premises on the CPU."""
import ctypes as C

import numpy as np
import pytest

from _arrays import DT, EPS, INTEGRATORS, LAYOUTS, SIZES, _dev, _dev_seq, _host_seq, _inf, _rollout, _wrench_rollout_inputs as _inputs, _wrenches
from _chains import WRENCH_CHAINS as CHAINS, _trio
from _components import _named_components as _components
from _feedback import (N_MULTI, T_MULTI, Law, _bound, _fb_rollout, _graded_gains, _limits, _multi_inputs, _np_closed_loop, _refs,
                       _sample_gains)
from _references import _oracle_fd

pytestmark = pytest.mark.gpu

MODES = [(integrator, hold) for integrator in INTEGRATORS for hold in (True, False)]
COMPONENT_CHAIN, TOOL_WRENCH_CHAINS = "ur10_like", ("panda_like", "ur10_public_long")   # (the latter: the chunked route with wrenches)


# ---- 1. one step rebuilt from the library's own evaluations
def _lib_eval(torch, chain, comps, W, link):
    """getJointAcceleration of the library at host arrays under the command u, whose entries are known to du -> ddq and the bound of the
    evaluation per sample: the solver term 64 eps cond2(M) max(1, |ddq|) plus the command's rounding carried through the solve,
    |M^-1|_2 |du|_2"""
    kw = {"components": comps}
    if W is not None:
        kw.update(ext_wrenches=torch.from_numpy(np.ascontiguousarray(W)).cuda(), ext_link=chain.getLinksName()[link])

    def fd(q, dq, u, du):
        tq, tdq = _dev(torch, q, "sample"), _dev(torch, dq, "sample")
        a, st = chain.getJointAcceleration(tq, tdq, _dev(torch, u, "sample"), **kw)
        assert (st.cpu().numpy() == 1).all()
        a = a.cpu().numpy()
        sv = np.linalg.svd(chain.getJointInertia(tq).cpu().numpy(), compute_uv=False)
        return a, 64.0 * EPS * sv[:, 0] / sv[:, -1] * np.maximum(1.0, _inf(a)) + np.sqrt((du * du).sum(axis=1)) / sv[:, -1]
    return fd


def _one_step_reference(fd, law, q0, dq0, integrator, hold):
    """(dq_ref, dq_bound, q_from or None, q_bound or a function of dq1): test_gpu_rollout_ext.py's one-step reference with the command
    formed in numpy -- at the start state for every stage under hold, at each stage's own state otherwise"""
    cmd = lambda q, dq: (law(0, q, dq), law.rounding(0, q, dq))
    held = cmd(q0, dq0)
    at = (lambda q, dq: held) if hold else cmd
    if integrator == "semi_implicit_euler":
        a, s = fd(q0, dq0, *held)
        return dq0 + DT * a, DT * s + 4 * EPS * (_inf(dq0) + DT * _inf(a)), None, lambda dq1: 4 * EPS * (_inf(q0) + DT * _inf(dq1))
    a1, s1 = fd(q0, dq0, *held)
    v2 = dq0 + 0.5 * DT * a1
    x2 = q0 + 0.5 * DT * dq0
    a2, s2 = fd(x2, v2, *at(x2, v2))
    v3 = dq0 + 0.5 * DT * a2
    x3 = q0 + 0.5 * DT * v2
    a3, s3 = fd(x3, v3, *at(x3, v3))
    v4 = dq0 + DT * a3
    x4 = q0 + DT * v3
    a4, s4 = fd(x4, v4, *at(x4, v4))
    dq_ref = dq0 + DT * (a1 / 6 + a2 / 3 + a3 / 3 + a4 / 6)
    dq_bound = DT * (s1 / 6 + s2 / 3 + s3 / 3 + s4 / 6) + 4 * EPS * (_inf(dq0) + DT * (_inf(a1) / 6 + _inf(a2) / 3 + _inf(a3) / 3 + _inf(a4) / 6))
    q_from = q0 + DT * (dq0 / 6 + v2 / 3 + v3 / 3 + v4 / 6)
    q_bound = DT * (0.5 * DT * s1 / 3 + 0.5 * DT * s2 / 3 + DT * s3 / 6) + 4 * EPS * (_inf(q0) + DT * (_inf(dq0) / 6 + _inf(v2) / 3 + _inf(v3) / 3 + _inf(v4) / 6))
    return dq_ref, dq_bound, q_from, q_bound


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_one_step_against_the_library_own_evaluations_in_closed_loop(name, integrator):
    """The form and the bounds of test_gpu_rollout_ext.py::test_one_step_against_the_library_own_evaluations_with_wrenches, the torque of
    every evaluation being the law's command formed in numpy.  The extra term: the command is two differences and two fused multiply-adds,
    so numpy's and the kernel's agree within du = 4 EPS (|tau_ff| + kp |e| + kd |de|) per entry (the clamp does not widen it: both sides
    lie within du of the limit where they disagree about it); through the solve that is at most |M^-1|_2 |du|_2 on ddq, added to the
    solver term of the evaluation.  Shared graded gains without limits and per-sample gains with limits, both modes; with components on
    one chain and the tool's wrench on two (one of them on the chunked route).  RK4 with the wrong mode misses the bound, and so does the
    rollout without feedback."""
    torch = pytest.importorskip("torch")
    chain, _, _ = _trio(name)
    n, L = chain.getActiveJointsNumber(), chain.getLinksNumber()
    comps = _components(name, n) if name == COMPONENT_CHAIN else None
    worst = 0.0
    for N in SIZES:
        q0, dq0, tau = _inputs(name, n, N, 1, seed=9100 + N)
        q_ref, dq_ref = _refs(q0, dq0, 1, seed=9120 + N)
        W = _wrenches(name, N, L, seed=9150 + N)[:, L - 1] if name in TOOL_WRENCH_CHAINS else None
        link = L - 1 if W is not None else None
        fd = _lib_eval(torch, chain, comps, W, link)
        laws = [Law(tau, q_ref, *_graded_gains(name, n), dq_ref=dq_ref),
                Law(tau, q_ref, *_sample_gains(name, n, N, seed=9170 + N), dq_ref=dq_ref, lim=_limits(name, n))]
        for law in laws:
            for hold in (True, False):
                dq_want, dq_bound, q_from, q_bound = _one_step_reference(fd, law, q0, dq0, integrator, hold)
                for layout in LAYOUTS:
                    q1, dq1, st = _fb_rollout(torch, chain, q0, dq0, law, integrator, layout, hold=hold, components=comps, W=W, link=link)
                    assert st.shape == (N,) and (st == 1).all(), np.unique(st)
                    edq = _inf(dq1 - dq_want)
                    if q_from is None:
                        eq, qb = _inf(q1 - (q0 + DT * dq1)), q_bound(dq1)
                    else:
                        eq, qb = _inf(q1 - q_from), q_bound
                    worst = max(worst, float((edq / dq_bound).max()), float((eq / qb).max()))
                    assert (edq <= dq_bound).all(), (layout, N, hold, float((edq / dq_bound).max()), int(np.argmax(edq / dq_bound)))
                    assert (eq <= qb).all(), (layout, N, hold, float((eq / qb).max()), int(np.argmax(eq / qb)))
                if N == 200:
                    if integrator == "rk4":   # the mode matters: the other one misses the same bound
                        _, dq_other, _ = _fb_rollout(torch, chain, q0, dq0, law, integrator, hold=not hold, components=comps, W=W, link=link)
                        assert (_inf(dq_other - dq_want) > dq_bound).any()
                    kw = {} if W is None else {"ext_wrenches": torch.from_numpy(np.ascontiguousarray(W)).cuda(), "ext_link": chain.getLinksName()[link]}
                    _, dq_plain, _ = _rollout(torch, chain, q0, dq0, tau, DT, integrator, components=comps, **kw)   # the feedback matters
                    assert (_inf(dq_plain - dq_want) > dq_bound).any()
    print("%s %s: err/bound max %.3g" % (name, integrator, worst))


# ---- 2., 3. multi-step against the oracle, without and with limits
_ORACLE = {}


def _oracle_run(ref, name, integrator, hold, limits):
    """the oracle's closed loop on the multi-step inputs, computed once per case and shared (Euler: one run for both modes)"""
    key = (name, integrator, hold or integrator == "semi_implicit_euler", limits)
    if key not in _ORACLE:
        q0, dq0, law = _multi_inputs(name, ref.n, limits)
        rec = []
        end = _np_closed_loop(_oracle_fd(ref), law, q0, dq0, T_MULTI, DT, integrator, key[2], rec)
        for x in end + tuple(r[2] for r in rec):
            x.setflags(write=False)
        _ORACLE[key] = (end, [r[2] for r in rec])
    return _ORACLE[key]


def _check_against_the_oracle(got, want, name, integrator, hold, what):
    scale = np.maximum(1.0, np.maximum(_inf(want[0]), _inf(want[1])))
    err = np.maximum(_inf(got[0] - want[0]), _inf(got[1] - want[1])) / scale
    bound = _bound(name, integrator, hold)
    print("%s %s hold=%d %s: err max %.3g (bound %.3g)" % (name, integrator, hold, what, err.max(), bound))
    assert (err <= bound).all(), (what, float(err.max()), bound, int(np.argmax(err)))


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("integrator,hold", MODES)
def test_multi_step_against_the_oracle_in_closed_loop(name, integrator, hold):
    """T = 8, N = 200, kp = 100 s, kd = 20 s per joint times the chain's recorded gain factor, references within +-0.5 of the initial
    state; the bound is 8 dev of _feedback.FB_MULTI_STEP."""
    torch = pytest.importorskip("torch")
    chain, ref, _ = _trio(name, oracle=True)
    q0, dq0, law = _multi_inputs(name, ref.n)
    q1, dq1, st = _fb_rollout(torch, chain, q0, dq0, law, integrator, hold=hold)
    assert (st == 1).all()
    _check_against_the_oracle((q1, dq1), _oracle_run(ref, name, integrator, hold, False)[0], name, integrator, hold, "no limits")


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("integrator,hold", MODES)
def test_saturation(name, integrator, hold):
    """The multi-step inputs with limits that clamp between 20 % and 80 % of the commands (asserted on the CPU from the oracle alone):
    the same bounds, and every command record whose unclamped oracle command exceeds the limit by more than 1e-9 relative is the limit
    itself, exactly."""
    torch = pytest.importorskip("torch")
    chain, ref, _ = _trio(name, oracle=True)
    q0, dq0, law = _multi_inputs(name, ref.n, limits=True)
    q1, dq1, st, _, _, ut = _fb_rollout(torch, chain, q0, dq0, law, integrator, hold=hold, trajectory_every=1, command_trajectory=True)
    assert (st == 1).all() and ut.shape == (T_MULTI, N_MULTI, ref.n)
    end, raw = _oracle_run(ref, name, integrator, hold, True)
    _check_against_the_oracle((q1, dq1), end, name, integrator, hold, "limits")
    raw = np.stack(raw)
    lim = np.broadcast_to(law.lim, raw.shape)
    above, below = raw > lim * (1.0 + 1e-9), raw < -lim * (1.0 + 1e-9)
    assert 0.2 <= (above | below).mean() <= 0.8
    assert np.array_equal(ut[above], lim[above]) and np.array_equal(ut[below], -lim[below])
    assert (np.abs(ut) <= lim).all()


# ---- 4. the command record
@pytest.mark.parametrize("name", ["ur10_like", "ur10_permuted", "rev14"])
@pytest.mark.parametrize("integrator,hold", MODES)
def test_the_command_record_is_the_law_at_the_state_before_the_step(name, integrator, hold):
    torch = pytest.importorskip("torch")
    chain, _, _ = _trio(name)
    n = chain.getActiveJointsNumber()
    for limits in (False, True):
        q0, dq0, law = _multi_inputs(name, n, limits)
        first = None
        for layout in LAYOUTS:
            r = _fb_rollout(torch, chain, q0, dq0, law, integrator, layout, hold=hold, trajectory_every=1, command_trajectory=True)
            qt, dqt, ut = r[3:]
            assert (r[2] == 1).all() and ut.shape == (T_MULTI, N_MULTI, n)
            for k in range(T_MULTI):
                q, dq = (q0, dq0) if k == 0 else (qt[k - 1], dqt[k - 1])
                err, tol = np.abs(ut[k] - law(k, q, dq)), law.rounding(k, q, dq)
                assert (err <= tol).all(), (layout, k, float((err / tol).max()))
            first = first or r
            assert all(np.array_equal(a, b) for a, b in zip(r, first)), layout   # the layouts give the same bits


@pytest.mark.parametrize("name", ["ur10_like", "rev14"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_decimated_command_record_writes_two_records_and_nothing_behind_them(name, layout):
    """traj_every = 3, T = 8: records 0 and 1 are the commands of steps 2 and 5 -- those of the full record -- and a poisoned buffer of
    four records keeps its last two; the command record alone is an output."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd._lib import INTEGRATORS as CODES, Batch, Feedback, RolloutDesc, check, lib
    chain, _, _ = _trio(name)
    n = chain.getActiveJointsNumber()
    q0, dq0, law = _multi_inputs(name, n, limits=True)
    gpu = lambda x: _dev_seq(torch, x, layout) if x.ndim == 3 else _dev(torch, x, layout)
    tq, tdq, ttau, tqr, tdqr = (gpu(x) for x in (q0, dq0, law.tau_ff, law.q_ref, law.dq_ref))
    tkp, tkd, tlim = (torch.from_numpy(x).cuda() for x in (law.kp, law.kd, law.lim))
    for integrator, hold in MODES:
        full = _fb_rollout(torch, chain, q0, dq0, law, integrator, layout, hold=hold, trajectory_every=1, command_trajectory=True)[5]
        poison = 777.0
        buf = torch.full((4,) + tuple(tq.shape), poison, dtype=torch.float64, device="cuda")
        b = Batch()
        b.n_samples, b.q, b.dq, b.ddq, b.layout, b.device = N_MULTI, tq.data_ptr(), tdq.data_ptr(), None, 1 if layout == "element" else 0, -1
        b.stream = torch.cuda.current_stream().cuda_stream
        d = RolloutDesc()
        d.n_steps, d.integrator, d.dt, d.tau, d.tau_step_stride = T_MULTI, CODES[integrator], DT, ttau.data_ptr(), n * N_MULTI
        d.traj_every, d.traj_step_stride = 3, n * N_MULTI
        f = Feedback()
        f.q_ref, f.dq_ref, f.ref_step_stride, f.kp, f.kd = tqr.data_ptr(), tdqr.data_ptr(), n * N_MULTI, tkp.data_ptr(), tkd.data_ptr()
        f.gains_per_sample, f.hold, f.tau_limit, f.tau_traj = 0, int(hold), tlim.data_ptr(), buf.data_ptr()
        nbytes = lib().rdyn_rollout_feedback_workspace_bytes(chain._h, C.byref(d), None, C.byref(f), N_MULTI, 0)
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device="cuda")
        check(lib().rdyn_rollout_feedback(chain._h, C.byref(b), C.byref(d), None, 0, None, C.byref(f), 0, ws.data_ptr(), nbytes))
        got = _host_seq(buf, layout)
        assert np.array_equal(got[0], full[2]) and np.array_equal(got[1], full[5]), (integrator, hold)
        assert (got[2:] == poison).all()


# ---- 5. bitwise self-consistency
def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", CHAINS)
def test_semi_implicit_euler_gives_the_same_bits_under_both_modes(name):
    torch = pytest.importorskip("torch")
    chain, _, _ = _trio(name)
    q0, dq0, law = _multi_inputs(name, chain.getActiveJointsNumber(), limits=True)
    run = lambda hold: _fb_rollout(torch, chain, q0, dq0, law, "semi_implicit_euler", hold=hold, trajectory_every=1, command_trajectory=True)
    a, b = run(True), run(False)
    assert (a[2] == 1).all() and _same(a, b)


@pytest.mark.parametrize("name", ["ur10_like", "mixed_joints", "rev10", "ur10_public_long", "rev14"])
@pytest.mark.parametrize("integrator,hold", MODES)
def test_the_horizon_splits_and_constant_or_repeated_inputs_are_the_same_call_bitwise(name, integrator, hold):
    torch = pytest.importorskip("torch")
    chain, _, _ = _trio(name)
    n, L, N, T = chain.getActiveJointsNumber(), chain.getLinksNumber(), N_MULTI, T_MULTI
    q0, dq0, law = _multi_inputs(name, n, limits=True)
    W = np.stack([_wrenches(name, N, L, seed=9410 + t) for t in range(T)])[:, :, L - 1]
    kw = dict(hold=hold, link=L - 1, wseq=True)
    whole = _fb_rollout(torch, chain, q0, dq0, law, integrator, W=W, **kw)
    assert (whole[2] == 1).all()
    # split at t0 = 3: the later call starts its torques, references and wrenches at its own step
    cut = lambda a, b: Law(law.tau_ff[a:b], law.q_ref[a:b], law.kp, law.kd, law.dq_ref[a:b], law.lim)
    q, dq, _ = _fb_rollout(torch, chain, q0, dq0, cut(0, 3), integrator, W=W[:3], **kw)
    part = _fb_rollout(torch, chain, q, dq, cut(3, T), integrator, W=W[3:], **kw)
    assert _same(part, whole)
    # element-major equals sample-major
    assert _same(_fb_rollout(torch, chain, q0, dq0, law, integrator, "element", W=W, **kw), whole)
    # a constant set point is the same set point repeated T times
    rep = lambda x: np.stack([x] * T)
    const = Law(law.tau_ff, law.q_ref[0], law.kp, law.kd, law.dq_ref[0], law.lim)
    same = Law(law.tau_ff, rep(law.q_ref[0]), law.kp, law.kd, rep(law.dq_ref[0]), law.lim)
    a = _fb_rollout(torch, chain, q0, dq0, const, integrator, hold=hold, trajectory_every=1, command_trajectory=True)
    assert _same(a, _fb_rollout(torch, chain, q0, dq0, same, integrator, hold=hold, trajectory_every=1, command_trajectory=True))
    assert not np.array_equal(a[0], whole[0])
    # per-sample gains that repeat the shared gains
    tiled = Law(law.tau_ff, law.q_ref, np.tile(law.kp, (N, 1)), np.tile(law.kd, (N, 1)), law.dq_ref, law.lim)
    for layout in LAYOUTS:
        assert _same(_fb_rollout(torch, chain, q0, dq0, tiled, integrator, layout, W=W, **kw), whole), layout
    # no velocity term: kd = None is kd = 0, and without it dq_ref is not needed
    nokd = _fb_rollout(torch, chain, q0, dq0, Law(law.tau_ff, law.q_ref, law.kp, None, None, law.lim), integrator, hold=hold)
    zero = _fb_rollout(torch, chain, q0, dq0, Law(law.tau_ff, law.q_ref, law.kp, 0.0 * law.kd, law.dq_ref, law.lim), integrator, hold=hold)
    assert _same(nokd, zero)
    with pytest.raises(ValueError, match="Input data dimensions mismatch"):   # fewer reference records than steps
        _fb_rollout(torch, chain, q0, dq0, Law(law.tau_ff, law.q_ref[:T - 1], law.kp, law.kd, law.dq_ref[:T - 1]), integrator, hold=hold)


@pytest.mark.parametrize("integrator,hold", MODES)
def test_chunk_size_does_not_change_the_result_in_closed_loop(integrator, hold):
    """rev14, chunk_samples 0 and 16384 + 64 at N = 16384 + 65: a full chunk and a single sample (the reasoning of
    test_gpu_rollout_ext.py::test_chunk_size_does_not_change_the_result_with_wrenches)."""
    torch = pytest.importorskip("torch")
    chain, _, _ = _trio("rev14")
    n, T, chunk = 14, 2, 16384 + 64
    N = chunk + 1
    q0, dq0, tau = _inputs("rev14", n, N, T, seed=9500)
    q_ref, dq_ref = _refs(q0, dq0, T, seed=9510)
    law = Law(tau, q_ref, *_sample_gains("rev14", n, N, seed=9520), dq_ref=dq_ref, lim=_limits("rev14", n))
    run = lambda c: _fb_rollout(torch, chain, q0, dq0, law, integrator, hold=hold, trajectory_every=1, command_trajectory=True, chunk_samples=c)
    a, b = run(0), run(chunk)
    assert (a[2] == 1).all() and len(a) == 6 and _same(a, b)


@pytest.mark.parametrize("name", ["ur10_like", "ur10_public_long", "rev14"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_without_feedback_the_new_entry_is_rollout_ext_bitwise(name, integrator):
    torch = pytest.importorskip("torch")
    from rosdyn_amd._lib import INTEGRATORS as CODES, Batch, ExtWrenches, RolloutDesc, check, lib
    chain, _, _ = _trio(name)
    n, L, N, T = chain.getActiveJointsNumber(), chain.getLinksNumber(), 200, 5
    q0, dq0, tau = _inputs(name, n, N, T, seed=9600)
    cs = _components(name, n) if name == "ur10_like" else None
    tq, tdq, ttau = _dev(torch, q0, "sample"), _dev(torch, dq0, "sample"), torch.from_numpy(tau).cuda()
    tw = torch.from_numpy(_wrenches(name, N, L, seed=9610)).cuda()
    for W in (None, tw):
        old = chain.rollout(tq, tdq, ttau, DT, integrator=integrator, components=cs, ext_wrenches=W)
        b = Batch()
        b.n_samples, b.q, b.dq, b.ddq, b.layout, b.device = N, tq.data_ptr(), tdq.data_ptr(), None, 0, -1
        b.stream = torch.cuda.current_stream().cuda_stream
        q1, dq1 = torch.full_like(tq, 777.0), torch.full_like(tq, 777.0)
        st = torch.zeros((N,), dtype=torch.int32, device="cuda")
        d = RolloutDesc()
        d.n_steps, d.integrator, d.dt, d.tau, d.tau_step_stride = T, CODES[integrator], DT, ttau.data_ptr(), n * N
        d.q_end, d.dq_end, d.status = q1.data_ptr(), dq1.data_ptr(), st.data_ptr()
        px = None
        if W is not None:
            x = ExtWrenches()
            x.w, x.link, x.step_stride = W.data_ptr(), -1, 0
            px = C.byref(x)
        nbytes = lib().rdyn_rollout_feedback_workspace_bytes(chain._h, C.byref(d), px, None, N, 0)
        assert nbytes == lib().rdyn_rollout_ext_workspace_bytes(chain._h, C.byref(d), px, N, 0)
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device="cuda")
        cp, k = chain._component_list(cs) if cs is not None else (None, 0)
        check(lib().rdyn_rollout_feedback(chain._h, C.byref(b), C.byref(d), cp, k, px, None, 0, ws.data_ptr(), nbytes))
        assert torch.equal(q1, old[0]) and torch.equal(dq1, old[1]) and torch.equal(st, old[2])


def test_a_closed_loop_rollout_replays_from_a_captured_graph():
    """tests/test_gpu_graph.py's pattern: first use outside capture, one capture on a single side stream, replays on fresh inputs in the
    captured buffers give the bits of the eager call."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd import Feedback
    chain, _, _ = _trio("ur10_like")
    n, N, T = chain.getActiveJointsNumber(), 5000, 4
    q, dq = (torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(2))
    tau = torch.rand((T, N, n), dtype=torch.float64, device="cuda") * 0.8 - 0.4
    q_ref, dq_ref = (torch.rand((T, N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(2))
    kp, kd, lim = (torch.full((n,), v, dtype=torch.float64, device="cuda") for v in (4.0, 0.8, 1.0))
    fb = Feedback(q_ref, kp, kd, dq_ref, hold=False, tau_limit=lim)
    q_end, dq_end = torch.empty_like(q), torch.empty_like(q)
    chain.rollout(q, dq, tau, DT, integrator="rk4", out=(q_end, dq_end), feedback=fb)   # first use outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            _, _, st = chain.rollout(q, dq, tau, DT, integrator="rk4", out=(q_end, dq_end), feedback=fb)
    for k in range(2):
        for x in (q, dq, q_ref, dq_ref):
            x.uniform_(-1, 1)
        tau.uniform_(-0.4, 0.4)
        q_end.zero_()
        dq_end.zero_()
        st.zero_()
        g.replay()
        torch.cuda.synchronize()
        q2, dq2, st2 = chain.rollout(q, dq, tau, DT, integrator="rk4", feedback=fb)
        assert torch.equal(q_end, q2) and torch.equal(dq_end, dq2) and torch.equal(st, st2) and bool((st == 1).all())


# ---- 6. status: a clamp must not launder NaN
@pytest.mark.parametrize("name", ["ur10_like", "rev14"])
@pytest.mark.parametrize("integrator,hold", MODES)
def test_a_nan_reference_or_gain_fails_its_sample_alone(name, integrator, hold):
    """q_ref of one sample is NaN at step 2 of 8, limits active: the command of step 2 is NaN (a clamp by fmin / fmax would make it a
    limit), the state after step 2 is NaN by propagation, the evaluation after it fails the pivot rule: status -1, the command records
    from step 2 on and the state records from step 2 on NaN, every earlier record and every other sample bit-identical to the clean run.
    The same for a NaN gain of one sample with per-sample gains, from the first step on."""
    torch = pytest.importorskip("torch")
    chain, _, _ = _trio(name)
    n, N, T, bad = chain.getActiveJointsNumber(), N_MULTI, T_MULTI, 37
    q0, dq0, law = _multi_inputs(name, n, limits=True)
    others = np.arange(N) != bad
    for layout in LAYOUTS:
        run = lambda l: _fb_rollout(torch, chain, q0, dq0, l, integrator, layout, hold=hold, trajectory_every=1, command_trajectory=True)
        clean = run(law)
        q_ref = law.q_ref.copy()
        q_ref[2, bad, n - 1] = np.nan
        q1, dq1, st, qt, dqt, ut = run(Law(law.tau_ff, q_ref, law.kp, law.kd, law.dq_ref, law.lim))
        assert st[bad] == -1 and (st[others] == 1).all()
        assert np.isnan(q1[bad]).all() and np.isnan(dq1[bad]).all()
        assert np.isnan(ut[2, bad, n - 1]) and np.isnan(ut[3:, bad]).all()
        assert np.isnan(qt[2, bad]).any() and np.isnan(qt[3:, bad]).all() and np.isnan(dqt[3:, bad]).all()
        for got, want in zip((q1, dq1), clean[:2]):
            assert np.array_equal(got[others], want[others])
        for got, want in zip((qt, dqt, ut), clean[3:]):
            assert np.array_equal(got[:, others], want[:, others]) and np.array_equal(got[:2, bad], want[:2, bad])
        kp = np.tile(law.kp, (N, 1))
        kp[bad, 0] = np.nan
        q1, dq1, st, qt, dqt, ut = run(Law(law.tau_ff, law.q_ref, kp, np.tile(law.kd, (N, 1)), law.dq_ref, law.lim))
        assert st[bad] == -1 and (st[others] == 1).all()
        assert np.isnan(q1[bad]).all() and np.isnan(ut[0, bad, 0]) and np.isnan(ut[1:, bad]).all() and np.isnan(qt[1:, bad]).all()
        for got, want in zip((q1, dq1), clean[:2]):
            assert np.array_equal(got[others], want[others])
        for got, want in zip((qt, dqt, ut), clean[3:]):
            assert np.array_equal(got[:, others], want[:, others])
