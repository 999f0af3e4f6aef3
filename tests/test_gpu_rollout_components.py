"""GPU tests of forward dynamics and rollouts with friction and spring components: rdyn_forward_dynamics_components /
Chain.getJointAcceleration(components=) and rdyn_rollout_components / Chain.rollout(components=),
    FD_c(q, dq, tau) = FD(q, dq, tau - tau_c(q, dq)),
tau_c what ComponentSet.getRegressor accumulates into a zero tau_add.  Sizes: N in {1, 63, 64, 65, 200}, T <= 8, dt = 1e-3; inputs from
uniform_pm1 with the torque scales of test_gpu_rollout.py.  Bounds hold per sample; no sample is excused."""
import os
import subprocess

import numpy as np
import pytest

from conftest import FIXTURES, ROOT
from _arrays import DT, EPS, INTEGRATORS, _dev, _host, _inf, _rollout, _rollout_inputs, _solve
from _chains import GRAV, _chain, _cpair
from _components import FRICTION1, FRICTION2, ROLLOUT_MIN_VELOCITY as MIN_VELOCITY, SPRING, _scaled_specs as _specs, _set
from _references import _np_rollout, _oracle_fd_c
from rosdyn_amd.urdf_gen import generated_revolute_chain

pytestmark = pytest.mark.gpu
# planar_2r: the smallest chain; ur10_like, panda_like: 6 and 7 joints; mixed_joints: prismatic joints; ur10_public_long: the reduced
# companion (are component indices still input indices?); ur10_permuted: input order differs from chain order; rev10: the largest
# register kernel; rev14, gen20_permuted: the chunked route, permuted
CHAINS = ["planar_2r", "ur10_like", "panda_like", "mixed_joints", "ur10_public_long", "ur10_permuted", "rev10", "rev14", "gen20_permuted"]
SIZES = (1, 63, 64, 65, 200)


def _inputs(name, n, N, T, seed):
    """test_gpu_rollout.py's inputs; ur10_permuted is ur10_like with its input joints permuted and takes its torque scale"""
    return _rollout_inputs("ur10_like" if name == "ur10_permuted" else name, n, N, T, seed=seed)


def _tau_add(torch, cs, q, dq):
    """the library's own component torque at host arrays (N, n): getRegressor into a zero tau_add"""
    tq, tdq = _dev(torch, q, "sample"), _dev(torch, dq, "sample")
    add = torch.zeros_like(tq)
    cs.getRegressor(tq, tdq, tau_add=add)
    return add.cpu().numpy()


# ---- 1. forward dynamics against the composition
@pytest.mark.parametrize("name", CHAINS)
def test_forward_dynamics_against_the_composition(name):
    """getJointAcceleration(components=cs) against getJointAcceleration(tau - tau_add): the two differ only in where the same subtraction
    happens, so the bound is the per-sample solver bound of test_gpu_forward_dynamics.py, 64 eps cond2(M) max(1, |ddq|), nothing added."""
    torch = pytest.importorskip("torch")
    chain, _ = _cpair(name, oracle=False)
    n = chain.getActiveJointsNumber()
    cs = _set(_specs(name, n), n)
    for N in SIZES:
        q, dq, tau = _inputs(name, n, N, 1, seed=6100 + N)
        tau = tau[0]
        add = _tau_add(torch, cs, q, dq)
        assert (np.abs(add).max(axis=0) > 0).sum() == min(n, 3)   # the joints with a component, and only they
        want, st = _solve(torch, chain, q, dq, tau - add, "sample")
        assert (st == 1).all()
        cond = np.linalg.cond(chain.getJointInertia(_dev(torch, q, "sample")).cpu().numpy())
        bound = 64.0 * EPS * cond * np.maximum(1.0, _inf(want))
        plain, _ = _solve(torch, chain, q, dq, tau, "sample")
        assert (_inf(plain - want) > bound).any()   # the components matter at this bound
        for layout in ("sample", "element"):
            got, st = _solve(torch, chain, q, dq, tau, layout, components=cs)
            assert st.shape == (N,) and (st == 1).all(), np.unique(st)
            err = _inf(got - want)
            print("%s %s N=%d: err/bound max %.3g" % (name, layout, N, (err / bound).max()))
            assert (err <= bound).all(), (layout, N, float((err / bound).max()), int(np.argmax(err / bound)))
            # ddq aliasing tau
            t = _dev(torch, tau, layout)
            out, st2 = chain.getJointAcceleration(_dev(torch, q, layout), _dev(torch, dq, layout), t, layout=layout, out=t, components=cs)
            assert out.data_ptr() == t.data_ptr() and np.array_equal(_host(t, layout), got) and (st2.cpu().numpy() == 1).all()


# ---- 2. no components is the old call, bitwise
@pytest.mark.parametrize("name", ["panda_like", "rev14"])
def test_no_components_is_the_old_call_bitwise(name):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N, T = chain.getActiveJointsNumber(), 200, 5
    none = _set([], n)
    q, dq, tau = _inputs(name, n, N, T, seed=6200)
    for layout in ("sample", "element"):
        a, sa = _solve(torch, chain, q, dq, tau[0], layout)
        b, sb = _solve(torch, chain, q, dq, tau[0], layout, components=none)
        assert np.array_equal(a, b) and np.array_equal(sa, sb) and (sa == 1).all()
        for integrator in INTEGRATORS:
            x = _rollout(torch, chain, q, dq, tau, DT, integrator, layout, trajectory_every=2)
            y = _rollout(torch, chain, q, dq, tau, DT, integrator, layout, trajectory_every=2, components=none)
            assert all(np.array_equal(u, v) for u, v in zip(x, y)) and (x[2] == 1).all()


# ---- 3. one step against the library's own pieces
def _lib_fd_c(torch, chain, cs):
    """test_gpu_rollout.py's _lib_fd with the component torque at the evaluation's own state subtracted first"""
    def fd(q, dq, tau):
        tq = _dev(torch, q, "sample")
        a, st = chain.getJointAcceleration(tq, _dev(torch, dq, "sample"), _dev(torch, tau - _tau_add(torch, cs, q, dq), "sample"))
        assert (st.cpu().numpy() == 1).all()
        a = a.cpu().numpy()
        cond = np.linalg.cond(chain.getJointInertia(tq).cpu().numpy())
        return a, 64.0 * EPS * cond * np.maximum(1.0, _inf(a))
    return fd


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_one_step_against_the_library_own_pieces(name, integrator):
    """The construction and the bounds of test_gpu_rollout.py::test_one_step_against_the_library_own_forward_dynamics, every stage's
    acceleration rebuilt as getJointAcceleration(tau - tau_add(stage state)): RK4 evaluates the components at the stage state (the old
    torques, or the step's initial state, miss these bounds by orders of magnitude: the component torques are of the order of tau)."""
    torch = pytest.importorskip("torch")
    chain, _ = _cpair(name, oracle=False)
    n = chain.getActiveJointsNumber()
    cs = _set(_specs(name, n), n)
    fd = _lib_fd_c(torch, chain, cs)
    for N in SIZES:
        q0, dq0, tau = _inputs(name, n, N, 1, seed=6300 + N)
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
        for layout in ("sample", "element"):
            q1, dq1, st = _rollout(torch, chain, q0, dq0, tau, DT, integrator, layout, components=cs)
            assert st.shape == (N,) and (st == 1).all(), np.unique(st)
            edq = _inf(dq1 - dq_ref)
            if q_from is None:
                eq, qb = _inf(q1 - (q0 + DT * dq1)), q_bound_of(dq1)
            else:
                eq, qb = _inf(q1 - q_from), q_bound
            print("%s %s %s N=%d: dq err/bound max %.3g, q err/bound max %.3g" % (name, integrator, layout, N, (edq / dq_bound).max(), (eq / qb).max()))
            assert (edq <= dq_bound).all(), (layout, N, float((edq / dq_bound).max()), int(np.argmax(edq / dq_bound)))
            assert (eq <= qb).all(), (layout, N, float((eq / qb).max()), int(np.argmax(eq / qb)))


# ---- 4. multi-step against the oracle


def _multi_step_inputs(name, n):
    return _inputs(name, n, 200, 8, seed=6400)


# Measured on the CPU with the oracle alone, on this test's own inputs (T = 8, N = 200, dt = 1e-3), the way MULTI_STEP of
# test_gpu_rollout.py was: the oracle rollout with components run plain and run with every ddq evaluation multiplied by (1 + 1e-11 xi), xi
# uniform in +-1 per entry (numpy default_rng(6401)).  dev = the largest deviation of the end state between the two, relative to
# max(1, |x|_inf) of the sample's (q, dq); the bound is 8 dev.  With every Coulomb parameter at full size dev exceeded 1e-9 on ur10_like (8.4e-9), panda_like
# (2.0e-9), mixed_joints (4.7e-8), ur10_public_long (6.1e-9) and rev14 (1.3e-9): COULOMB shrinks theirs to 0.3, the first of 1, 0.3, 0.1, ...
# at which the oracle alone stays below 1e-9 for both integrators.  The factor 8 is not loosened.
MULTI_STEP_C = {
    # (chain, integrator): (dev, bound = 8 dev)
    ("planar_2r", "semi_implicit_euler"): (1.97e-12, 1.58e-11),
    ("planar_2r", "rk4"): (6.86e-13, 5.49e-12),
    ("ur10_like", "semi_implicit_euler"): (9.26e-11, 7.41e-10),
    ("ur10_like", "rk4"): (9.04e-12, 7.23e-11),
    ("panda_like", "semi_implicit_euler"): (2.95e-11, 2.36e-10),
    ("panda_like", "rk4"): (7.1e-12, 5.68e-11),
    ("mixed_joints", "semi_implicit_euler"): (3.8e-11, 3.04e-10),
    ("mixed_joints", "rk4"): (6.67e-12, 5.34e-11),
    ("ur10_public_long", "semi_implicit_euler"): (1.8e-11, 1.44e-10),
    ("ur10_public_long", "rk4"): (6.98e-12, 5.58e-11),
    ("ur10_permuted", "semi_implicit_euler"): (1.75e-11, 1.4e-10),
    ("ur10_permuted", "rk4"): (1.05e-11, 8.4e-11),
    ("rev10", "semi_implicit_euler"): (9.76e-11, 7.81e-10),
    ("rev10", "rk4"): (7.09e-11, 5.67e-10),
    ("rev14", "semi_implicit_euler"): (8.65e-12, 6.92e-11),
    ("rev14", "rk4"): (5.05e-12, 4.04e-11),
    ("gen20_permuted", "semi_implicit_euler"): (7.67e-12, 6.14e-11),
    ("gen20_permuted", "rk4"): (3.86e-12, 3.09e-11),
}


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_multi_step_against_the_oracle(name, integrator):
    torch = pytest.importorskip("torch")
    chain, ref = _cpair(name)
    specs = _specs(name, ref.n)
    q0, dq0, tau = _multi_step_inputs(name, ref.n)
    q1, dq1, st = _rollout(torch, chain, q0, dq0, tau, DT, integrator, components=_set(specs, ref.n))
    assert (st == 1).all()
    qr, dqr = _np_rollout(_oracle_fd_c(ref, specs), q0, dq0, tau, DT, 8, integrator)
    scale = np.maximum(1.0, np.maximum(_inf(qr), _inf(dqr)))
    err = np.maximum(_inf(q1 - qr), _inf(dq1 - dqr)) / scale
    bound = MULTI_STEP_C[(name, integrator)][1]
    print("%s %s: err max %.3g (bound %.3g)" % (name, integrator, err.max(), bound))
    assert (err <= bound).all(), (float(err.max()), bound, int(np.argmax(err)))


# ---- 5. closed form
def _rev1_zero_gravity():
    from rosdyn_amd import Chain
    return Chain(generated_revolute_chain(1, 1001), "l0", "l1", (0.0, 0.0, 0.0))


def _scalar_rk4(f, x, v, dt, T):
    """classical RK4 of x' = v, v' = f(x, v) in numpy (arrays over the samples)"""
    for _ in range(T):
        a1 = f(x, v)
        v2 = v + 0.5 * dt * a1
        a2 = f(x + 0.5 * dt * v, v2)
        v3 = v + 0.5 * dt * a2
        a3 = f(x + 0.5 * dt * v2, v3)
        v4 = v + dt * a3
        a4 = f(x + dt * v3, v4)
        x, v = x + dt * (v / 6 + v2 / 3 + v3 / 3 + v4 / 6), v + dt * (a1 / 6 + a2 / 3 + a3 / 3 + a4 / 6)
    return x, v


@pytest.mark.parametrize("case", ["spring", "viscous"])
def test_closed_form_on_one_joint(case):
    """rev1, zero gravity, tau = 0, RK4, T = 8, dt = 1e-3, N = 200; M read from getJointInertia (one joint: constant, h = 0).
    spring {k, off}: q(t) = q_eq + (q0 - q_eq) cos wt + (Dq0 / w) sin wt, q_eq = -off / k, w^2 = k / M, with k = M 50^2 (w dt = 0.05).
    viscous-only FRICTION1 {0, b}, max_velocity 2 > |Dq0|: Dq(t) = Dq0 exp(-b t / M), q(t) = q0 + Dq0 (M / b) (1 - exp(-b t / M)), b = 50 M.
    Tolerance, measured in the test itself: 8 x the largest error over the samples of a numpy RK4 of the same scalar ODE against the closed
    form at the same dt and T, plus 16 eps max(1, |x|) per sample, x = (q, Dq)."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd.samples import uniform_pm1
    chain = _rev1_zero_gravity()
    N, T = 200, 8
    q0, dq0 = uniform_pm1(6500, (N, 1)), uniform_pm1(6501, (N, 1))
    M = chain.getJointInertia(_dev(torch, q0, "sample")).cpu().numpy().reshape(N)
    assert np.ptp(M) <= 4 * EPS * M.max() and M.min() > 0
    M = float(M[0])
    t = T * DT
    if case == "spring":
        w = 50.0
        k, off = M * w * w, 0.3 * M * w * w
        specs = [(SPRING, 0, 0.0, 0.0, (k, off, 0.0))]
        q_eq = -off / k
        q_x = q_eq + (q0 - q_eq) * np.cos(w * t) + dq0 / w * np.sin(w * t)
        dq_x = -(q0 - q_eq) * w * np.sin(w * t) + dq0 * np.cos(w * t)
        f = lambda x, v: -(k * x + off) / M
    else:
        lam = 50.0
        b = lam * M
        specs = [(FRICTION1, 0, MIN_VELOCITY, 2.0, (0.0, b, 0.0))]
        dq_x = dq0 * np.exp(-lam * t)
        q_x = q0 + dq0 / lam * (1.0 - np.exp(-lam * t))
        f = lambda x, v: -(b * v) / M
    q_n, dq_n = _scalar_rk4(f, q0, dq0, DT, T)
    scheme = max(np.abs(q_n - q_x).max(), np.abs(dq_n - dq_x).max())
    q1, dq1, st = _rollout(torch, chain, q0, dq0, np.zeros((N, 1)), DT, "rk4", n_steps=T, components=_set(specs, 1))
    assert (st == 1).all()
    tol = 8.0 * scheme + 16.0 * EPS * np.maximum(1.0, np.maximum(_inf(q_x), _inf(dq_x)))
    err = np.maximum(_inf(q1 - q_x), _inf(dq1 - dq_x))
    print("%s: M %.3g, numpy RK4 error %.3g, err max %.3g, err/tol max %.3g" % (case, M, scheme, err.max(), (err / tol).max()))
    assert scheme > 0 and (err <= tol).all(), (float((err / tol).max()), int(np.argmax(err / tol)))
    plain = _rollout(torch, chain, q0, dq0, np.zeros((N, 1)), DT, "rk4", n_steps=T)
    assert (np.maximum(_inf(plain[0] - q_x), _inf(plain[1] - dq_x)) > tol).any()   # without the component the closed form is missed


# ---- 6. structure inherited from the rollout
@pytest.mark.parametrize("name", ["ur10_permuted", "rev14"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_the_horizon_can_be_split_anywhere_bitwise(name, integrator):
    torch = pytest.importorskip("torch")
    chain, _ = _cpair(name, oracle=False)
    n, N, T = chain.getActiveJointsNumber(), 200, 7
    cs = _set(_specs(name, n), n)
    q0, dq0, tau = _inputs(name, n, N, T, seed=6600)
    whole = _rollout(torch, chain, q0, dq0, tau, DT, integrator, components=cs)
    assert (whole[2] == 1).all() and np.isfinite(whole[0]).all() and np.isfinite(whole[1]).all()
    assert not np.array_equal(whole[0], _rollout(torch, chain, q0, dq0, tau, DT, integrator)[0])
    for cuts in ([1] * 7, [3, 4]):
        q, dq, t0, worst = q0, dq0, 0, np.ones(N, dtype=np.int32)
        for k in cuts:
            q, dq, st = _rollout(torch, chain, q, dq, tau[t0:t0 + k], DT, integrator, components=cs)
            worst = np.minimum(worst, st)
            t0 += k
        assert np.array_equal(q, whole[0]) and np.array_equal(dq, whole[1]) and np.array_equal(worst, whole[2]), cuts
    el = _rollout(torch, chain, q0, dq0, tau, DT, integrator, "element", components=cs)
    assert all(np.array_equal(a, b) for a, b in zip(el, whole))


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_chunk_size_does_not_change_the_result(integrator):
    torch = pytest.importorskip("torch")
    chain = _chain("rev14")
    n, N, T = 14, 200, 3
    cs = _set(_specs("rev14", n), n)
    q0, dq0, tau = _inputs("rev14", n, N, T, seed=6700)
    a = _rollout(torch, chain, q0, dq0, tau, DT, integrator, trajectory_every=1, components=cs, chunk_samples=0)
    for layout in ("sample", "element"):
        b = _rollout(torch, chain, q0, dq0, tau, DT, integrator, layout, trajectory_every=1, components=cs, chunk_samples=(N + 2) // 3)
        assert (a[2] == 1).all() and all(np.array_equal(x, y) for x, y in zip(a, b))
    fa, _ = _solve(torch, chain, q0, dq0, tau[0], "sample", components=cs)
    fb, _ = _solve(torch, chain, q0, dq0, tau[0], "element", components=cs, chunk_samples=(N + 2) // 3)
    assert np.array_equal(fa, fb)


@pytest.mark.parametrize("name", ["ur10_permuted", "rev14"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_trajectory_records_match_chained_calls(name, integrator):
    torch = pytest.importorskip("torch")
    chain, _ = _cpair(name, oracle=False)
    n, N, T = chain.getActiveJointsNumber(), 200, 7
    cs = _set(_specs(name, n), n)
    q0, dq0, tau = _inputs(name, n, N, T, seed=6800)
    ends = [_rollout(torch, chain, q0, dq0, tau, DT, integrator, n_steps=k, components=cs) for k in range(1, T + 1)]
    for layout in ("sample", "element"):
        for every in (1, 3):
            q1, dq1, st, qt, dqt = _rollout(torch, chain, q0, dq0, tau, DT, integrator, layout, trajectory_every=every, components=cs)
            assert qt.shape == (T // every, N, n) and (st == 1).all()
            assert np.array_equal(q1, ends[T - 1][0]) and np.array_equal(dq1, ends[T - 1][1])
            for k in range(T // every):
                assert np.array_equal(qt[k], ends[(k + 1) * every - 1][0]) and np.array_equal(dqt[k], ends[(k + 1) * every - 1][1]), (layout, every, k)


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("layout", ["sample", "element"])
def test_failure_reports_minus_one_and_nan_from_the_failing_step_on(integrator, layout):
    """The fixture of test_gpu_rollout.py: ur10_public with the fixed joint of tool0 among the input joints (its row and column of M are
    zero) -- every sample fails at the first step; a valid chain with the same components afterwards is untouched."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd import Chain
    chain = Chain(os.path.join(FIXTURES, "ur10_public.urdf"), "base_link", "tool0", GRAV)
    moving = ["shoulder_pan_joint", "shoulder_lift_joint", "elbow_joint", "wrist_1_joint", "wrist_2_joint", "wrist_3_joint"]
    assert chain.setInputJointsName(moving[:3] + ["flange-tool0"] + moving[3:])
    n, N, T = 7, 200, 3
    cs = _set(_specs("ur10_like", n), n)
    q0, dq0, tau = _inputs("ur10_like", n, N, T, seed=6900)
    q1, dq1, st, qt, dqt = _rollout(torch, chain, q0, dq0, tau, DT, integrator, layout, trajectory_every=1, components=cs)
    assert (st == -1).all() and np.isnan(q1).all() and np.isnan(dq1).all()
    assert qt.shape == (T, N, n) and np.isnan(qt).all() and np.isnan(dqt).all()
    ddq, st = _solve(torch, chain, q0, dq0, tau[0], layout, components=cs)
    assert (st == -1).all() and np.isnan(ddq).all()
    good = _chain("panda_like")
    r = _rollout(torch, good, q0, dq0, tau, DT, integrator, layout, components=cs)
    assert (r[2] == 1).all() and np.isfinite(r[0]).all() and np.isfinite(r[1]).all()


@pytest.mark.parametrize("name", ["ur10_like", "rev14"])
def test_replays_from_a_captured_graph(name):
    """a linear graph (one stream, no parallel branches); the first call is made outside capture"""
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N, T = chain.getActiveJointsNumber(), 200, 4
    cs = _set(_specs(name, n), n)
    rounds = [_inputs(name, n, N, T, seed=7000 + 10 * k) for k in range(3)]   # the first call's inputs, then one set per replay
    q, dq, tau = (torch.from_numpy(x).cuda() for x in rounds[0])
    q_end, dq_end = torch.empty_like(q), torch.empty_like(q)
    ws = torch.empty((max(1, chain_workspace(chain, N, T)),), dtype=torch.uint8, device="cuda")
    chain.rollout(q, dq, tau, DT, integrator="rk4", out=(q_end, dq_end), workspace=ws, components=cs)   # first use outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            _, _, st = chain.rollout(q, dq, tau, DT, integrator="rk4", out=(q_end, dq_end), workspace=ws, components=cs)
    for q_k, dq_k, tau_k in rounds[1:]:
        q.copy_(torch.from_numpy(q_k))
        dq.copy_(torch.from_numpy(dq_k))
        tau.copy_(torch.from_numpy(tau_k))
        q_end.zero_()
        dq_end.zero_()
        g.replay()
        torch.cuda.synchronize()
        q2, dq2, st2 = chain.rollout(q, dq, tau, DT, integrator="rk4", components=cs)
        assert torch.equal(q_end, q2) and torch.equal(dq_end, dq2) and torch.equal(st, st2) and bool((st == 1).all())
        assert not torch.equal(q_end, chain.rollout(q, dq, tau, DT, integrator="rk4")[0])


def chain_workspace(chain, N, T):
    import ctypes as C
    from rosdyn_amd._lib import INTEGRATORS as CODES, RolloutDesc, lib
    d = RolloutDesc()
    d.n_steps, d.integrator, d.dt = T, CODES["rk4"], DT
    return lib().rdyn_rollout_workspace_bytes(chain._h, C.byref(d), N, 0)


# ---- 7. the C++ facade
def test_facade_with_components(tmp_path):
    """tests/cpp/rollout_components_facade.cpp (built with -Wall -Wextra -Werror -pedantic, run once per chain): getJointAccelerationBatch and
    rolloutBatch with a leading component list and the single-sample getJointAcceleration(q, Dq, tau, comps), on ur10_like and on a
    generated 14-joint chain; inputs are exact binary fractions, its numbers equal the Python binding's to 1e-13."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd import Chain
    exe = tmp_path / "rollout_components_facade"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "rosdyn_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "rollout_components_facade.cpp"),
                           "-o", str(exe), "-L" + os.path.join(ROOT, "rosdyn_amd"), "-lrdyn_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "rosdyn_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    long_urdf = tmp_path / "rev14.urdf"
    long_urdf.write_text(generated_revolute_chain(14, 1014))
    for urdf, base, tool in ((os.path.join(FIXTURES, "ur10_like.urdf"), "base_link", "tool0"), (str(long_urdf), "l0", "l14")):
        r = subprocess.run([str(exe), urdf, base, tool], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout + r.stderr
        got = {line.split()[0]: np.array([float(x) for x in line.split()[1:]]) for line in r.stdout.splitlines() if line != "ok"}
        chain = Chain(urdf, base, tool, GRAV)
        n, N, T = chain.getActiveJointsNumber(), 5, 3
        s, i = np.meshgrid(np.arange(N), np.arange(n), indexing="ij")
        value = lambda k: ((s * 7 + i * 3 + k * 5) % 17 - 8) / 16.0
        q, dq, tau = value(0), value(1), np.stack([0.5 * value(2 + t) for t in range(T)])
        cs = _set([(FRICTION1, 0, 0.0625, 0.75, (0.25, 0.5, 0.0)), (FRICTION2, n - 1, 0.0625, 0.75, (0.125, 0.25, -0.5)),
                   (SPRING, 0, 0.0, 0.0, (1.5, -0.25, 0.0))], n)
        ddq, st = _solve(torch, chain, q, dq, tau[0], "sample", components=cs)
        q1, dq1, st1 = _rollout(torch, chain, q, dq, tau, 1e-3, "rk4", components=cs)
        assert (st == 1).all() and (st1 == 1).all()
        for key, want in (("ddq", ddq), ("q_end", q1), ("dq_end", dq1), ("single", ddq[0])):
            assert got[key].shape == (want.size,) and np.abs(got[key] - want.reshape(-1)).max() <= 1e-13, key
