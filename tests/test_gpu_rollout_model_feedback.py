"""GPU tests of the model-based laws of the closed-loop rollouts, rdyn_rollout_model_feedback / Chain.rollout(feedback=ModelFeedback):
    computed torque        a = ddq_ref + kp (q_ref - q) + kd (Dq_ref - Dq),  u = clamp(tau_ff + RNEA_m(q, Dq, a))
    gravity compensation   u = clamp(tau_ff + kp (q_ref - q) + kd (Dq_ref - Dq) + RNEA_m(q, 0, 0))
with a WRONG model everywhere (every inertial parameter off by up to 6.25 %, Chain.withParameters).  Checked against (1) the command of
one step from the oracle's regressor and from the library's own getJointTorque of the model, (2) the CPU oracle run through the same law
and integrators in numpy, (3) a closed form that needs neither, (4) the same as (2) with limits that clamp a fair share of the commands,
(5) itself, bitwise, (6) the oracle with plant components and with a tool wrench, (7) the status rule, (8) a captured graph, (9) the
refusal of the chunked route.  N = 200 (three full waves and a partial one), T = 8, dt = 1e-3.
The inputs, the laws in numpy and the tables of measured bounds are tests/_model_feedback.py's; tests/test_rollout_model_feedback_inputs.py
pins them on the CPU."""
import ctypes as C

import numpy as np
import pytest

from _arrays import DT, INTEGRATORS, LAYOUTS, _dev, _dev_seq, _inf, _wrenches
from _chains import _trio
from _components import _named_components as _components, _scaled_specs
from _feedback import N_MULTI, T_MULTI, Law, _fb_rollout, _np_closed_loop
from _model_feedback import (CHAINS, CT, GC, LAWS, MF_CLOSED_FORM, ModelLaw, _closed_form_end, _closed_form_inputs, _mf_bound, _mf_inputs, _mfb_rollout,
                             _model, _model_torque, _near_a_limit, _with_torque)
from _references import _oracle_fd, _oracle_fd_c, _oracle_fd_ext

pytestmark = pytest.mark.gpu

MODES = [(integrator, hold) for integrator in INTEGRATORS for hold in (True, False)]
COMPONENT_CHAIN, TOOL_WRENCH_CHAIN = "ur10_like", "panda_like"
_SETUP, _ORACLE = {}, {}


def _setup(name):
    """(chain, oracle chain, the model chain with the wrong parameters, the same model without gravity), once per chain"""
    if name not in _SETUP:
        chain, ref, chain0 = _trio(name, oracle=True)
        _SETUP[name] = (chain, ref, _model(chain), _model(chain0))
    return _SETUP[name]


def _oracle_run(ref, name, integrator, hold, law, limits=False, per_sample=False):
    """the oracle's closed loop on the multi-step inputs, computed once per case and shared (Euler: one run for both modes): (end state,
    record, ModelLaw)"""
    key = (name, integrator, hold or integrator == "semi_implicit_euler", law, limits, per_sample)
    if key not in _ORACLE:
        q0, dq0, l = _mf_inputs(ref, name, law, limits, per_sample)
        rec = []
        end = _np_closed_loop(_oracle_fd(ref), l, q0, dq0, T_MULTI, DT, integrator, key[2], rec)
        for x in end:
            x.setflags(write=False)
        _ORACLE[key] = (end, rec, l)
    return _ORACLE[key]


def _state_error(got, want):
    scale = np.maximum(1.0, np.maximum(_inf(want[0]), _inf(want[1])))
    return np.maximum(_inf(got[0] - want[0]), _inf(got[1] - want[1])) / scale


# ---- 1. one step: the command record
@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("law", LAWS)
def test_the_command_of_one_step_is_the_law_with_the_model_torque(name, law):
    """T = 1, no limits: the command record against tau_ff + Y(q0, dq0, a) pi_hat from the oracle and against the library's own
    model.getJointTorque(q0, dq0, a), a formed in numpy (gravity compensation: the PD command + the torque at v = a = 0).  Both within the
    project's parity bound, 1e-11 relative to max(1, |u|_inf) of the sample; both layouts, shared and per-sample gains."""
    torch = pytest.importorskip("torch")
    chain, ref, model, _ = _setup(name)
    for per_sample in (False, True):
        q0, dq0, l = _mf_inputs(ref, name, law, per_sample=per_sample)
        want, tau_m = l.terms(0, q0, dq0)
        want = want + tau_m
        if law == CT:
            a = l._pd(0, q0, dq0) + l.ddq_ref[0]
            lib_m = model.getJointTorque(*(_dev(torch, x, "sample") for x in (q0, dq0, a))).cpu().numpy()
        else:
            tq = _dev(torch, q0, "sample")
            lib_m = model.getJointTorque(tq, torch.zeros_like(tq), torch.zeros_like(tq)).cpu().numpy()
        want_lib = (want - tau_m) + lib_m
        scale = np.maximum(1.0, _inf(want))
        for layout in LAYOUTS:
            for integrator, hold in MODES:
                r = _mfb_rollout(torch, chain, model, q0, dq0, l, integrator, layout, hold=hold, n_steps=1, trajectory_every=1, command_trajectory=True)
                assert (r[2] == 1).all() and r[5].shape == (1, N_MULTI, ref.n)
                eo, el = _inf(r[5][0] - want) / scale, _inf(r[5][0] - want_lib) / scale
                assert (eo <= 1e-11).all() and (el <= 1e-11).all(), (layout, integrator, hold, float(eo.max()), float(el.max()))
        print("%s %s per_sample=%d: oracle %.3g library %.3g" % (name, law, per_sample, eo.max(), el.max()))
        # the model matters: the plant's own parameters miss the bound
        exact = _with_torque(l, _model_torque(ref, ref.nominal_parameters())).raw(0, q0, dq0)
        assert (_inf(r[5][0] - exact) / scale > 1e-11).any()


# ---- 2. multi-step against the oracle loop
@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("integrator,hold", MODES)
@pytest.mark.parametrize("law", LAWS)
def test_multi_step_against_the_oracle_loop(name, integrator, hold, law):
    """T = 8, N = 200, shared and per-sample gains; the bound is 8 dev of _model_feedback.MF_MULTI_STEP."""
    torch = pytest.importorskip("torch")
    chain, ref, model, _ = _setup(name)
    bound = _mf_bound(name, integrator, hold, law)
    for per_sample in (False, True):
        end, _, l = _oracle_run(ref, name, integrator, hold, law, per_sample=per_sample)
        q0, dq0, _ = _mf_inputs(ref, name, law, per_sample=per_sample)
        q1, dq1, st = _mfb_rollout(torch, chain, model, q0, dq0, l, integrator, hold=hold)
        assert (st == 1).all()
        err = _state_error((q1, dq1), end)
        print("%s %s hold=%d %s per_sample=%d: err max %.3g (bound %.3g)" % (name, integrator, hold, law, per_sample, err.max(), bound))
        assert (err <= bound).all(), (per_sample, float(err.max()), bound, int(np.argmax(err)))


# ---- 3. the closed form
@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_the_exact_model_follows_the_closed_form_of_the_error_dynamics(name, integrator):
    """model = the chain itself, computed torque, no limits, tau_ff = 0, a constant set point: q'' = a up to rounding, so every joint's
    error obeys e'' + kd e' + kp e = 0 under the integrator's own linear map (_model_feedback._closed_form_end).  hold = 0; bound: 8
    times the deviation of the oracle's own loop from the recurrence (MF_CLOSED_FORM)."""
    torch = pytest.importorskip("torch")
    chain, ref, _, _ = _setup(name)
    q0, dq0, q_ref, kp, kd = _closed_form_inputs(name, ref.n)
    law = ModelLaw(None, CT, np.zeros_like(q0), q_ref, kp, kd)
    q1, dq1, st = _mfb_rollout(torch, chain, chain, q0, dq0, law, integrator, hold=False, n_steps=T_MULTI)
    assert (st == 1).all()
    err = _state_error((q1, dq1), _closed_form_end(q0, dq0, q_ref, kp, kd, integrator))
    bound = 8.0 * MF_CLOSED_FORM[(name, integrator)]
    print("%s %s: err max %.3g (bound %.3g)" % (name, integrator, err.max(), bound))
    assert (err <= bound).all(), (float(err.max()), bound, int(np.argmax(err)))


# ---- 4. saturation
@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("integrator,hold", MODES)
@pytest.mark.parametrize("law", LAWS)
def test_saturation(name, integrator, hold, law):
    """Limits that clamp between 20 % and 80 % of the commands (LIMIT_FACTOR_CT): command records and end state within the bound of the
    multi-step test; samples in which a raw command of the oracle lies within the law's rounding of a limit are left out of the
    comparison, at most 5 % of them."""
    torch = pytest.importorskip("torch")
    chain, ref, model, _ = _setup(name)
    end, rec, l = _oracle_run(ref, name, integrator, hold, law, limits=True)
    q0, dq0, _ = _mf_inputs(ref, name, law, limits=True)
    q1, dq1, st, _, _, ut = _mfb_rollout(torch, chain, model, q0, dq0, l, integrator, hold=hold, trajectory_every=1, command_trajectory=True)
    assert (st == 1).all() and ut.shape == (T_MULTI, N_MULTI, ref.n)
    raw, u = np.stack([r[2] for r in rec]), np.stack([r[3] for r in rec])
    assert 0.2 <= (raw != u).mean() <= 0.8
    assert (np.abs(ut) <= l.lim).all()
    keep = ~_near_a_limit(rec, l)
    assert keep.mean() >= 0.95
    bound = _mf_bound(name, integrator, hold, law)
    err = _state_error((q1[keep], dq1[keep]), (end[0][keep], end[1][keep]))
    eu = np.abs(ut - u)[:, keep].max(axis=(0, 2)) / np.maximum(1.0, np.abs(u)[:, keep].max(axis=(0, 2)))
    print("%s %s hold=%d %s: state %.3g command %.3g (bound %.3g), %d samples left out" % (name, integrator, hold, law, err.max(), eu.max(), bound,
                                                                                          (~keep).sum()))
    assert (err <= bound).all(), (float(err.max()), bound)
    assert (eu <= bound).all(), (float(eu.max()), bound)


# ---- 5. bitwise identities
def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("integrator,hold", MODES)
@pytest.mark.parametrize("law", LAWS)
def test_layouts_split_horizons_and_repeated_runs_give_the_same_bits(name, integrator, hold, law):
    torch = pytest.importorskip("torch")
    chain, ref, model, model0 = _setup(name)
    q0, dq0, l = _mf_inputs(ref, name, law, limits=True)
    kw = dict(hold=hold, trajectory_every=1, command_trajectory=True)
    whole = _mfb_rollout(torch, chain, model, q0, dq0, l, integrator, **kw)
    assert (whole[2] == 1).all()
    assert _same(_mfb_rollout(torch, chain, model, q0, dq0, l, integrator, **kw), whole)              # two runs
    assert _same(_mfb_rollout(torch, chain, model, q0, dq0, l, integrator, "element", **kw), whole)   # the layouts
    # a horizon split at step 3: the later call starts its torques and references, ddq_ref among them, at its own step
    cut = lambda a, b: ModelLaw(None, law, l.tau_ff[a:b], l.q_ref[a:b], l.kp, l.kd, l.dq_ref[a:b], None if l.ddq_ref is None else l.ddq_ref[a:b], l.lim)
    first = _mfb_rollout(torch, chain, model, q0, dq0, cut(0, 3), integrator, **kw)
    second = _mfb_rollout(torch, chain, model, first[0], first[1], cut(3, T_MULTI), integrator, **kw)
    assert _same(second[:3], whole[:3])
    for k in (3, 4, 5):
        assert np.array_equal(np.concatenate([first[k], second[k]]), whole[k])
    if integrator == "semi_implicit_euler" and hold:   # one computation under both modes
        assert _same(_mfb_rollout(torch, chain, model, q0, dq0, l, integrator, hold=False, trajectory_every=1, command_trajectory=True), whole)
    if law == GC:   # a model without gravity adds a signed zero: the PD call's bits
        pd = _fb_rollout(torch, chain, q0, dq0, Law(l.tau_ff, l.q_ref, l.kp, l.kd, l.dq_ref, l.lim), integrator, **kw)
        assert _same(_mfb_rollout(torch, chain, model0, q0, dq0, l, integrator, **kw), pd)
        assert not np.array_equal(pd[0], whole[0])


@pytest.mark.parametrize("name", ["ur10_like", "ur10_public"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_without_a_model_law_the_new_entry_is_rollout_feedback_bitwise(name, integrator):
    torch = pytest.importorskip("torch")
    from rosdyn_amd._lib import INTEGRATORS as CODES, Batch, Feedback, RolloutDesc, check, lib
    chain, ref, _, _ = _setup(name)
    n, N, T = ref.n, N_MULTI, T_MULTI
    q0, dq0, l = _mf_inputs(ref, name, GC, limits=True)
    old = _fb_rollout(torch, chain, q0, dq0, Law(l.tau_ff, l.q_ref, l.kp, l.kd, l.dq_ref, l.lim), integrator, hold=False)
    tq, tdq = _dev(torch, q0, "sample"), _dev(torch, dq0, "sample")
    ttau, tqr, tdqr = (_dev_seq(torch, x, "sample") for x in (l.tau_ff, l.q_ref, l.dq_ref))
    tkp, tkd, tlim = (torch.from_numpy(x).cuda() for x in (l.kp, l.kd, l.lim))
    b = Batch()
    b.n_samples, b.q, b.dq, b.ddq, b.layout, b.device = N, tq.data_ptr(), tdq.data_ptr(), None, 0, -1
    b.stream = torch.cuda.current_stream().cuda_stream
    q1, dq1 = torch.full_like(tq, 777.0), torch.full_like(tq, 777.0)
    st = torch.zeros((N,), dtype=torch.int32, device="cuda")
    d = RolloutDesc()
    d.n_steps, d.integrator, d.dt, d.tau, d.tau_step_stride = T, CODES[integrator], DT, ttau.data_ptr(), n * N
    d.q_end, d.dq_end, d.status = q1.data_ptr(), dq1.data_ptr(), st.data_ptr()
    f = Feedback()
    f.q_ref, f.dq_ref, f.ref_step_stride, f.kp, f.kd = tqr.data_ptr(), tdqr.data_ptr(), n * N, tkp.data_ptr(), tkd.data_ptr()
    f.gains_per_sample, f.hold, f.tau_limit = 0, 0, tlim.data_ptr()
    nbytes = lib().rdyn_rollout_model_feedback_workspace_bytes(chain._h, C.byref(d), None, C.byref(f), None, N, 0)
    assert nbytes == lib().rdyn_rollout_feedback_workspace_bytes(chain._h, C.byref(d), None, C.byref(f), N, 0)
    check(lib().rdyn_rollout_model_feedback(chain._h, C.byref(b), C.byref(d), None, 0, None, C.byref(f), None, 0, None, 0))
    assert np.array_equal(q1.cpu().numpy(), old[0]) and np.array_equal(dq1.cpu().numpy(), old[1]) and np.array_equal(st.cpu().numpy(), old[2])


# ---- 6. plant components and a tool wrench behind the clamp
@pytest.mark.parametrize("integrator,hold", MODES)
def test_with_plant_components_against_the_oracle_loop(integrator, hold):
    torch = pytest.importorskip("torch")
    name = COMPONENT_CHAIN
    chain, ref, model, _ = _setup(name)
    q0, dq0, l = _mf_inputs(ref, name, CT, limits=True)
    comps = _components(name, ref.n)
    want = _np_closed_loop(_oracle_fd_c(ref, _scaled_specs(name, ref.n)), l, q0, dq0, T_MULTI, DT, integrator, hold)
    q1, dq1, st = _mfb_rollout(torch, chain, model, q0, dq0, l, integrator, hold=hold, components=comps)
    assert (st == 1).all()
    err, bound = _state_error((q1, dq1), want), _mf_bound(name, integrator, hold, CT)
    print("%s %s hold=%d components: err max %.3g (bound %.3g)" % (name, integrator, hold, err.max(), bound))
    assert (err <= bound).all(), (float(err.max()), bound)
    assert (_state_error(_mfb_rollout(torch, chain, model, q0, dq0, l, integrator, hold=hold)[:2], want) > bound).any()   # they matter


@pytest.mark.parametrize("integrator,hold", MODES)
def test_with_a_tool_wrench_against_the_oracle_loop(integrator, hold):
    torch = pytest.importorskip("torch")
    name = TOOL_WRENCH_CHAIN
    chain, ref, model, _ = _setup(name)
    L = chain.getLinksNumber()
    q0, dq0, l = _mf_inputs(ref, name, CT, limits=True)
    W = np.zeros((N_MULTI, L, 6))
    W[:, L - 1] = _wrenches(name, N_MULTI, L, seed=9810)[:, L - 1]
    want = _np_closed_loop(_oracle_fd_ext(ref, W), l, q0, dq0, T_MULTI, DT, integrator, hold)
    q1, dq1, st = _mfb_rollout(torch, chain, model, q0, dq0, l, integrator, hold=hold, W=W[:, L - 1], link=L - 1)
    assert (st == 1).all()
    err, bound = _state_error((q1, dq1), want), _mf_bound(name, integrator, hold, CT)
    print("%s %s hold=%d tool wrench: err max %.3g (bound %.3g)" % (name, integrator, hold, err.max(), bound))
    assert (err <= bound).all(), (float(err.max()), bound)
    assert (_state_error(_mfb_rollout(torch, chain, model, q0, dq0, l, integrator, hold=hold)[:2], want) > bound).any()   # it matters


# ---- 7. status
@pytest.mark.parametrize("name", ["ur10_like", "rev10"])
@pytest.mark.parametrize("integrator,hold", MODES)
def test_a_nan_acceleration_reference_fails_its_sample_alone_and_no_steps_copy_the_state(name, integrator, hold):
    torch = pytest.importorskip("torch")
    chain, ref, model, _ = _setup(name)
    n, N, bad = ref.n, N_MULTI, 37
    q0, dq0, l = _mf_inputs(ref, name, CT, limits=True)
    others = np.arange(N) != bad
    for layout in LAYOUTS:
        run = lambda law, **kw: _mfb_rollout(torch, chain, model, q0, dq0, law, integrator, layout, hold=hold, **kw)
        clean = run(l, trajectory_every=1, command_trajectory=True)
        ddq_ref = l.ddq_ref.copy()
        ddq_ref[2, bad, n - 1] = np.nan
        q1, dq1, st, qt, dqt, ut = run(ModelLaw(None, CT, l.tau_ff, l.q_ref, l.kp, l.kd, l.dq_ref, ddq_ref, l.lim), trajectory_every=1,
                                       command_trajectory=True)
        assert st[bad] == -1 and (st[others] == 1).all()
        assert np.isnan(q1[bad]).all() and np.isnan(dq1[bad]).all()
        assert np.isnan(ut[2, bad]).any() and np.isnan(ut[3:, bad]).all()
        assert np.isnan(qt[2, bad]).any() and np.isnan(qt[3:, bad]).all() and np.isnan(dqt[3:, bad]).all()
        for got, want in zip((q1, dq1), clean[:2]):
            assert np.array_equal(got[others], want[others])
        for got, want in zip((qt, dqt, ut), clean[3:]):
            assert np.array_equal(got[:, others], want[:, others]) and np.array_equal(got[:2, bad], want[:2, bad])
        q1, dq1, st = run(l, n_steps=0)
        assert np.array_equal(q1, q0) and np.array_equal(dq1, dq0) and (st == 1).all()


# ---- 8. a captured graph
@pytest.mark.parametrize("law", LAWS)
def test_a_model_based_rollout_replays_from_a_captured_graph(law):
    """tests/test_gpu_graph.py's pattern: first use outside capture (both chains), one capture on a side stream, the replay gives the bits
    of the eager call."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd import ModelFeedback
    chain, ref, model, _ = _setup("ur10_like")
    q0, dq0, l = _mf_inputs(ref, "ur10_like", law, limits=True)
    seq = lambda x: None if x is None else _dev_seq(torch, x, "sample")
    q, dq, tau = _dev(torch, q0, "sample"), _dev(torch, dq0, "sample"), seq(l.tau_ff)
    fb = ModelFeedback(model, law, seq(l.q_ref), *(torch.from_numpy(x).cuda() for x in (l.kp, l.kd)), seq(l.dq_ref), seq(l.ddq_ref), hold=False,
                       tau_limit=torch.from_numpy(l.lim).cuda())
    q_end, dq_end = torch.empty_like(q), torch.empty_like(q)
    chain.rollout(q, dq, tau, DT, integrator="rk4", out=(q_end, dq_end), feedback=fb)   # first use outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            _, _, st = chain.rollout(q, dq, tau, DT, integrator="rk4", out=(q_end, dq_end), feedback=fb)
    q.uniform_(-1, 1)
    dq.uniform_(-1, 1)
    q_end.zero_()
    dq_end.zero_()
    st.zero_()
    g.replay()
    torch.cuda.synchronize()
    q2, dq2, st2 = chain.rollout(q, dq, tau, DT, integrator="rk4", feedback=fb)
    assert torch.equal(q_end, q2) and torch.equal(dq_end, dq2) and torch.equal(st, st2) and bool((st == 1).all())


# ---- 9. the chunked route
def test_the_chunked_route_is_refused():
    torch = pytest.importorskip("torch")
    from rosdyn_amd import RdynError
    chain, ref, _ = _trio("rev14", oracle=True)
    model = _model(chain)
    q0, dq0, l = _mf_inputs(ref, "rev14", CT)
    with pytest.raises(RdynError, match="RDYN_ERR_UNSUPPORTED.*chunked route"):
        _mfb_rollout(torch, chain, model, q0, dq0, l, "rk4")
