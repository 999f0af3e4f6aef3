"""Seeded structural fuzz (-m gpu) of the three dynamics entry points the older fuzz does not reach: rdyn_forward_dynamics,
rdyn_joint_torque_derivatives and rdyn_rollout on the random chains of test_gpu_fuzz.py (1 .. 10 chain joints, every joint kind, fixed
joints anywhere, missing <origin>/<axis>/<inertial>, side branches, sub-paths, random gravity, permuted subsets of the input joints; the
same chain, gravity and subset per seed as test_fuzzed_chain_all_entry_points) against the CPU oracle.  N = 257: four full waves, whose
sample-major records leave through the staged path, and a ragged lane.

Every sample is classified from the oracle alone (classify): regular -- the smallest eigenvalue of M_ref is at least 1e-8 trace(M_ref),
a hundred times the kernels' 1e-10 trace rule and a lower bound of every pivot in any elimination order -- or singular -- a diagonal
entry of M_ref at most 1e-14 trace(M_ref), or a zero trace.  A sample in neither class fails the test; none is excused.
tests/test_fuzz_dynamics_inputs.py pins, without a GPU, what these tests rest on.
tests/test_gpu_fuzz_gradients.py runs the entry points merged since on the same cases: components, derivatives, VJP, rollout adjoint.

Bounds, each per sample:
  forward dynamics   the residual bound of test_gpu_forward_dynamics.py (1e-11) against the oracle and its 64 eps cond2 solver bound
                     against a host solve of the library's own M and h; singular samples report -1 and NaN
  derivatives        the exact reference of test_gpu_torque_derivatives.py, its construction gap (1e-12) asserted first, 1e-11 of
                     max|D_ref| + |tau_ref|_inf per entry
  rollouts           T = 4, dt = 1e-3, both integrators: the one-step residual check of test_gpu_rollout.py; the end state against the numpy
                     rollout over the oracle within rollout_bound(), computed at run time from the oracle alone by the definition above
                     MULTI_STEP in test_gpu_rollout.py; a horizon cut into [1, 3] steps gives the same bits
  input subsets      the full chain with the unselected joints held at q = dq = 0 (forward dynamics: and at ddq = 0, by the oracle's
                     holding torque) gives the subset chain's outputs on the selected joints: the same bits for the derivatives, the
                     64 eps cond2 solver bound for ddq."""
import numpy as np
import pytest

from _arrays import EPS, INTEGRATORS, PRISMATIC, _dev, _host, _inf, _mat, _rollout
from _fuzz import DT, FUZZ_OFFSET, N, T, _chain, _get, _regular_neighbour, case, classify, reference_derivatives, rollout_bound, seed_class
from _references import _euler_residual_check, _input_types, _solver_bound_check

pytestmark = pytest.mark.gpu


def _fd(torch, chain, q, dq, tau, layout):
    ddq, st = chain.getJointAcceleration(_dev(torch, q, layout), _dev(torch, dq, layout), _dev(torch, tau, layout), layout=layout)
    return _host(ddq, layout), st.cpu().numpy()


def _forward_dynamics_regular(torch, c, chain, what):
    ddq, st = _fd(torch, chain, c.q, c.dq, c.tau, c.layout)
    assert st.shape == (N,) and (st == 1).all(), np.unique(st)
    assert np.isfinite(ddq).all()
    res = _inf(np.einsum("sij,sj->si", c.M, ddq) + c.h - c.tau)
    scale = np.abs(c.M).sum(axis=2).max(axis=1) * _inf(ddq) + _inf(c.tau) + _inf(c.h)
    print("%s: residual ratio max %.3g (bound 1e-11), lambda_min / trace >= %.3g" % (what, (res / scale).max(), c.lam.min()))
    assert (res <= 1e-11 * scale).all(), (float((res / scale).max()), int(np.argmax(res / scale)))
    tq, tdq = _dev(torch, c.q, "sample"), _dev(torch, c.dq, "sample")
    M = chain.getJointInertia(tq).cpu().numpy()
    h = chain.getJointTorqueNonLinearPart(tq, tdq).cpu().numpy()
    _solver_bound_check(ddq, M, h, c.tau, what)
    return ddq


@pytest.mark.parametrize("seed", range(64))
def test_forward_dynamics(seed):
    torch = pytest.importorskip("torch")
    c = _get(seed)
    kind = seed_class(c)
    chain = _chain(c)
    what = "seed %d (nJ %d, n %d, %s, %s)" % (seed, c.ref.nJ, c.n, "subset" if c.inputs else "all inputs", c.layout)
    if kind == "regular":
        _forward_dynamics_regular(torch, c, chain, what)
        return
    ddq, st = _fd(torch, chain, c.q, c.dq, c.tau, c.layout)
    assert st.shape == (N,) and (st == -1).all(), np.unique(st)
    assert ddq.shape == (N, c.n) and np.isnan(ddq).all()
    print("%s: singular, status -1 and NaN on all %d samples" % (what, N))
    good = _regular_neighbour(seed)
    _forward_dynamics_regular(torch, good, _chain(good), "seed %d after the singular seed %d" % (good.seed, seed))


LIGHT = 2.0 ** -40


@pytest.mark.parametrize("seed", [5, 17])
def test_locked_joints_stay_out_of_the_pivot_rule(seed):
    """The pivot rule is relative to the trace of the INPUT joints' block of M.  Seeds 5 and 17 lock 2 of 4 and 5 of 7 moveable joints; with
    every mass and inertia tensor scaled by 2^-40 the traces are of order 1e-12 while lambda_min / trace stays what it was (the scaling is
    exact), so the samples are regular by the same rule -- and a unit diagonal of a locked joint counted in the trace would put the floor,
    1e-10 (trace + 1), above every pivot.  (On the unscaled seeds the traces are 2e-2 at the least and the pivots 4e-4 of them: there the
    same error changes no status.)"""
    torch = pytest.importorskip("torch")
    if FUZZ_OFFSET:
        pytest.skip("seeds chosen among the committed ones")
    c, plain = case(seed, LIGHT), case(seed)
    assert c.inputs is not None and len(c.inputs) < c.full.n and c.inputs == plain.inputs
    assert seed_class(c) == "regular" and np.array_equal(c.M, LIGHT * plain.M)
    assert np.einsum("sii->s", c.M).max() < 1e-10   # no pivot exceeds the trace: all of them lie below a floor of 1e-10 (trace + 1)
    _forward_dynamics_regular(torch, c, _chain(c), "seed %d, inertias x 2^-40 (trace <= %.3g)" % (seed, np.einsum("sii->s", c.M).max()))


@pytest.mark.parametrize("seed", range(64))
def test_torque_derivatives(seed):
    torch = pytest.importorskip("torch")
    c = _get(seed)
    chain = _chain(c)
    types = _input_types(chain)
    assert types == c.oracle_types()
    Dq_ref, Dv_ref, tau_ref, gap = reference_derivatives(c)
    scale = np.maximum(_inf(Dq_ref), _inf(Dv_ref)) + _inf(tau_ref)
    tiny = np.finfo(np.float64).tiny
    print("seed %d: construction gap %.3g (bound 1e-12)" % (seed, float((gap / np.maximum(scale, tiny)).max())))
    assert (gap <= 1e-12 * scale).all(), ("spectral reference, 8 against 16 points", float((gap / np.maximum(scale, tiny)).max()))
    out = chain.getJointTorqueDerivatives(_dev(torch, c.q, c.layout), _dev(torch, c.dq, c.layout), _dev(torch, c.ddq, c.layout),
                                          layout=c.layout, want=("dq", "dv", "M"))
    worst = {}
    for what, t, want in (("dtau_dq", out[0], Dq_ref), ("dtau_dv", out[1], Dv_ref), ("M", out[2], c.M)):
        got = _mat(t, c.layout)
        assert got.shape == (N, c.n, c.n) and np.isfinite(got).all(), what
        sc = _inf(want) + _inf(tau_ref)
        err = _inf(got - want)
        worst[what] = float((err / np.maximum(sc, tiny)).max())
        assert (err <= 1e-11 * sc).all(), (what, worst[what], int(np.argmax(err / np.maximum(sc, tiny))))
    print("seed %d (nJ %d, n %d, %s, %s, %d prismatic): worst ratio dtau_dq %.3g dtau_dv %.3g M %.3g (bound 1e-11)"
          % (seed, c.ref.nJ, c.n, "subset" if c.inputs else "all inputs", c.layout, types.count(PRISMATIC), worst["dtau_dq"], worst["dtau_dv"],
             worst["M"]))


@pytest.mark.parametrize("seed", range(64))
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_rollout(seed, integrator):
    torch = pytest.importorskip("torch")
    c = _get(seed)
    kind = seed_class(c)
    chain = _chain(c)
    what = "seed %d %s (nJ %d, n %d, %s, %s)" % (seed, integrator, c.ref.nJ, c.n, "subset" if c.inputs else "all inputs", c.layout)
    if kind == "singular":
        q1, dq1, st, qt, dqt = _rollout(torch, chain, c.q, c.dq, c.tau_seq, DT, integrator, c.layout, trajectory_every=1)
        assert st.shape == (N,) and (st == -1).all(), np.unique(st)
        assert q1.shape == (N, c.n) and np.isnan(q1).all() and np.isnan(dq1).all()
        assert qt.shape == (T, N, c.n) and np.isnan(qt).all() and np.isnan(dqt).all()
        print("%s: singular, status -1 and NaN in the end state and all %d records" % (what, T))
        return
    if integrator == "semi_implicit_euler":
        _euler_residual_check(torch, chain, c.ref, what, N, c.layout, None, inputs=(c.q, c.dq, c.tau_seq[:1]))
    bound, dev, qr, dqr = rollout_bound(c, integrator)
    assert np.isfinite(bound) and bound > 0.0
    q1, dq1, st = _rollout(torch, chain, c.q, c.dq, c.tau_seq, DT, integrator, c.layout)
    assert st.shape == (N,) and (st == 1).all(), np.unique(st)
    scale = np.maximum(1.0, np.maximum(_inf(qr), _inf(dqr)))
    err = np.maximum(_inf(q1 - qr), _inf(dq1 - dqr)) / scale
    print("%s: end-state err max %.3g (run-time bound %.3g = 8 x %.3g), ratio %.3g" % (what, err.max(), bound, dev, err.max() / bound))
    assert (err <= bound).all(), (float(err.max()), bound, int(np.argmax(err)))
    # the horizon cut into [1, 3] steps: the same bits
    qa, dqa, sta = _rollout(torch, chain, c.q, c.dq, c.tau_seq[:1], DT, integrator, c.layout)
    qb, dqb, stb = _rollout(torch, chain, qa, dqa, c.tau_seq[1:], DT, integrator, c.layout)
    assert np.array_equal(qb, q1) and np.array_equal(dqb, dq1) and np.array_equal(np.minimum(sta, stb), st)
    assert not np.array_equal(q1, c.q)


@pytest.mark.parametrize("seed", range(64))
def test_input_subset_against_the_full_chain(seed):
    """The subset chain locks its unselected moveable joints at 0; the full chain, given 0 there, evaluates the same functions."""
    torch = pytest.importorskip("torch")
    c = _get(seed)
    kind = seed_class(c)
    if c.inputs is None or kind != "regular":
        return   # nothing to compare: every moveable joint is an input joint, or the subset chain itself is singular (the tests above)
    sub, full = _chain(c), _chain(c, subset=False)
    pos = c.positions_in_full()
    qf, dqf, ddqf = c.scatter(c.q), c.scatter(c.dq), c.scatter(c.ddq)
    dev = lambda x: _dev(torch, x, c.layout)
    a = sub.getJointTorqueDerivatives(dev(c.q), dev(c.dq), dev(c.ddq), layout=c.layout, want=("dq", "dv", "M"))
    b = full.getJointTorqueDerivatives(dev(qf), dev(dqf), dev(ddqf), layout=c.layout, want=("dq", "dv", "M"))
    for what, x, y in zip(("dtau_dq", "dtau_dv", "M"), a, b):
        x, y = _mat(x, c.layout), _mat(y, c.layout)[:, pos][:, :, pos]
        assert np.array_equal(x, y), (what, float(np.abs(x - y).max()))
    # forward dynamics: the unselected joints get the torque that holds them at ddq = 0 (the oracle's), the selected ones the subset's
    Mf = c.full.joint_inertia(qf)
    regular, singular, lam = classify(Mf)
    assert (regular | singular).all() and (regular.all() or singular.all()), "the full chain classifies too"
    tauf = c.full.joint_torque(qf, dqf, c.scatter(c.a))
    tauf[:, pos] = c.tau
    ddq_full, st_full = _fd(torch, full, qf, dqf, tauf, c.layout)
    what = "seed %d (nJ %d, %d of %d moveable joints selected)" % (seed, c.ref.nJ, c.n, c.full.n)
    if singular.all():
        # a massless tail behind an unselected joint: the subset chain is regular, the full chain is not, and says so
        assert (st_full == -1).all() and np.isnan(ddq_full).all()
        print("%s: derivatives bitwise; the full chain is singular (-1 and NaN), no ddq to compare" % what)
        return
    ddq_sub, st_sub = _fd(torch, sub, c.q, c.dq, c.tau, c.layout)
    assert (st_sub == 1).all() and (st_full == 1).all()
    cond = np.linalg.cond(Mf)
    ratio = _inf(ddq_full[:, pos] - ddq_sub) / (EPS * cond * np.maximum(1.0, _inf(ddq_sub)))
    print("%s: derivatives bitwise, ddq ratio max %.3g (bound 64), cond2 of the full chain %.3g .. %.3g" % (what, ratio.max(), cond.min(), cond.max()))
    assert (ratio <= 64.0).all(), (float(ratio.max()), int(np.argmax(ratio)))
