"""GPU tests of the batched rollouts rdyn_rollout / Chain.rollout: T steps of semi-implicit Euler or classical RK4 over the forward
dynamics ddq = FD(q, dq, tau_t), torques held over a step.  The reference has no integrator: the call is defined by rdyn_forward_dynamics
plus a textbook integrator, and checked against (a) the library's own getJointAcceleration, one step, (b) the CPU oracle's joint_inertia /
joint_torque run through the same integrator in numpy.  Bounds hold per sample; no sample is excused."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import FIXTURES, ROOT
from _arrays import DT, EPS, INTEGRATORS, REV_EXTRA, _dev, _dev_seq, _host, _inf, _rollout, _rollout_inputs as _inputs
from _chains import GRAV, _chain, _pair
from _references import _euler_residual_check, _np_rollout, _oracle_fd
from rosdyn_amd.urdf_gen import generated_revolute_chain

pytestmark = pytest.mark.gpu
CHAINS = ["planar_2r", "ur10_like", "panda_like", "mixed_joints", "ur10_public_long", "rev10", "rev14", "gen20_permuted"]


# ---- the same integrators in numpy over any forward dynamics fd(q, dq, tau) -> ddq


# ---- 1. one step against what already exists
def _lib_fd(torch, chain):
    """getJointAcceleration, getJointInertia of the library on host arrays -> ddq, the solver term 64 eps cond2(M) max(1, |ddq|) per sample"""
    def fd(q, dq, tau):
        tq, tdq = _dev(torch, q, "sample"), _dev(torch, dq, "sample")
        a, st = chain.getJointAcceleration(tq, tdq, _dev(torch, tau, "sample"))
        assert (st.cpu().numpy() == 1).all()
        a = a.cpu().numpy()
        cond = np.linalg.cond(chain.getJointInertia(tq).cpu().numpy())
        return a, 64.0 * EPS * cond * np.maximum(1.0, _inf(a))
    return fd


@pytest.mark.parametrize("name", CHAINS + REV_EXTRA)
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_one_step_against_the_library_own_forward_dynamics(name, integrator):
    """Euler: |dq1 - dq0 - dt ddq_lib| <= dt 64 eps cond2(M) max(1, |ddq_lib|) + 4 eps (|dq0| + dt |ddq_lib|) (the solver bound of
    test_gpu_forward_dynamics.py plus two roundings of the update), |q1 - q0 - dt dq1| <= 4 eps (|q0| + dt |dq1|).  RK4: the four stages
    rebuilt in numpy from four getJointAcceleration calls at the stage states; the per-stage bounds summed with the RK4 weights (the stage
    velocity v_i = dq0 + c_i dt a_{i-1} carries c_i dt times the solver term of a_{i-1} into q1)."""
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    fd = _lib_fd(torch, chain)
    for N in (1, 63, 64, 65, 200):
        q0, dq0, tau = _inputs(name, n, N, 1, seed=4100 + N)
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
            q1, dq1, st = _rollout(torch, chain, q0, dq0, tau, DT, integrator, layout)
            assert st.shape == (N,) and (st == 1).all(), np.unique(st)
            edq = _inf(dq1 - dq_ref)
            if q_from is None:
                eq, qb = _inf(q1 - (q0 + DT * dq1)), q_bound_of(dq1)
            else:
                eq, qb = _inf(q1 - q_from), q_bound
            print("%s %s %s N=%d: dq err/bound max %.3g, q err/bound max %.3g" % (name, integrator, layout, N, (edq / dq_bound).max(), (eq / qb).max()))
            assert (edq <= dq_bound).all(), (layout, N, float((edq / dq_bound).max()), int(np.argmax(edq / dq_bound)))
            assert (eq <= qb).all(), (layout, N, float((eq / qb).max()), int(np.argmax(eq / qb)))


# ---- 2. one Euler step against the oracle, residual form


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("layout", ["sample", "element"])
def test_one_euler_step_against_the_oracle_in_residual_form(name, layout):
    """With ddq := (dq1 - dq0) / dt: |M_ref ddq + h_ref - tau| <= 1e-11 scale + (4 eps / dt) (|dq0| + dt |ddq|) |M_ref|_inf, scale as in
    test_gpu_forward_dynamics.py::test_against_the_oracle_in_residual_form."""
    torch = pytest.importorskip("torch")
    chain, ref = _pair(name)
    _euler_residual_check(torch, chain, ref, name, 200, layout, 4300)


# ---- 3. the horizon can be split anywhere, bitwise
@pytest.mark.parametrize("name", ["ur10_like", "mixed_joints", "ur10_public_long", "rev10", "rev14", "gen20_permuted"] + REV_EXTRA)
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_the_horizon_can_be_split_anywhere_bitwise(name, integrator):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N, T = chain.getActiveJointsNumber(), 200, 7
    q0, dq0, tau = _inputs(name, n, N, T, seed=4400)
    whole = _rollout(torch, chain, q0, dq0, tau, DT, integrator)
    assert (whole[2] == 1).all() and np.isfinite(whole[0]).all() and np.isfinite(whole[1]).all()
    assert not np.array_equal(whole[0], q0)
    for cuts in ([1] * 7, [3, 4]):
        q, dq, t0, worst = q0, dq0, 0, np.ones(N, dtype=np.int32)
        for k in cuts:
            q, dq, st = _rollout(torch, chain, q, dq, tau[t0:t0 + k], DT, integrator)
            worst = np.minimum(worst, st)
            t0 += k
        assert np.array_equal(q, whole[0]) and np.array_equal(dq, whole[1]) and np.array_equal(worst, whole[2]), cuts
    # element-major equals sample-major
    el = _rollout(torch, chain, q0, dq0, tau, DT, integrator, "element")
    assert all(np.array_equal(a, b) for a, b in zip(el, whole))


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_chunk_size_does_not_change_the_result(integrator):
    torch = pytest.importorskip("torch")
    chain = _chain("rev14")
    n, N, T = 14, 4000, 3
    q0, dq0, tau = _inputs("rev14", n, N, T, seed=4500)
    a = _rollout(torch, chain, q0, dq0, tau, DT, integrator, trajectory_every=1)
    b = _rollout(torch, chain, q0, dq0, tau, DT, integrator, trajectory_every=1, chunk_samples=(N + 2) // 3)
    c = _rollout(torch, chain, q0, dq0, tau, DT, integrator, "element", trajectory_every=1, chunk_samples=1000)
    assert (a[2] == 1).all()
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and all(np.array_equal(x, y) for x, y in zip(a, c))


# ---- 4. multi-step against the oracle
# Measured on the CPU with the oracle alone, on this test's own inputs (T = 8, N = 200, dt = 1e-3): the oracle rollout run plain and run with
# every ddq evaluation multiplied by (1 + 1e-11 xi), xi uniform in +-1 per entry (1e-11: the project's parity figure).  dev = the largest
# deviation of the end state between the two, relative to max(1, |x|_inf) of the sample's (q, dq); the bound is 8 dev (a random perturbation
# under-samples the worst case).  max|ddq| = the largest acceleration the plain run saw.
MULTI_STEP = {
    # (chain, integrator): (dev, bound = 8 dev, max|ddq|)
    ("planar_2r", "semi_implicit_euler"): (1.23e-12, 9.88e-12, 53.3),
    ("planar_2r", "rk4"): (6.79e-13, 5.44e-12, 53.3),
    ("ur10_like", "semi_implicit_euler"): (2.66e-11, 2.13e-10, 793),
    ("ur10_like", "rk4"): (1.3e-11, 1.04e-10, 793),
    ("panda_like", "semi_implicit_euler"): (1.46e-11, 1.17e-10, 732),
    ("panda_like", "rk4"): (7.45e-12, 5.96e-11, 732),
    ("mixed_joints", "semi_implicit_euler"): (1.93e-11, 1.54e-10, 645),
    ("mixed_joints", "rk4"): (1.14e-11, 9.13e-11, 645),
    ("ur10_public_long", "semi_implicit_euler"): (1.72e-11, 1.38e-10, 740),
    ("ur10_public_long", "rk4"): (6.69e-12, 5.35e-11, 740),
    ("rev10", "semi_implicit_euler"): (7.34e-12, 5.87e-11, 481),
    ("rev10", "rk4"): (4.31e-12, 3.45e-11, 481),
    ("rev14", "semi_implicit_euler"): (1.03e-11, 8.23e-11, 475),
    ("rev14", "rk4"): (3.91e-12, 3.13e-11, 475),
    ("gen20_permuted", "semi_implicit_euler"): (7.63e-12, 6.1e-11, 300),
    ("gen20_permuted", "rk4"): (3.99e-12, 3.19e-11, 300),
}


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_multi_step_against_the_oracle(name, integrator):
    torch = pytest.importorskip("torch")
    chain, ref = _pair(name)
    N, T = 200, 8
    q0, dq0, tau = _inputs(name, ref.n, N, T, seed=4600)
    q1, dq1, st = _rollout(torch, chain, q0, dq0, tau, DT, integrator)
    assert (st == 1).all()
    qr, dqr = _np_rollout(_oracle_fd(ref), q0, dq0, tau, DT, T, integrator)
    scale = np.maximum(1.0, np.maximum(_inf(qr), _inf(dqr)))
    err = np.maximum(_inf(q1 - qr), _inf(dq1 - dqr)) / scale
    bound = MULTI_STEP[(name, integrator)][1]
    print("%s %s: err max %.3g (bound %.3g)" % (name, integrator, err.max(), bound))
    assert (err <= bound).all(), (float(err.max()), bound, int(np.argmax(err)))


# ---- 5. order of the integrators
# Chosen on the CPU with the oracle's own integrators (constant torques, N = 64, reference: oracle RK4 at dt / 8):
ORDER = {
    # chain: (span, dt, torque amplitude, oracle ratio rk4, oracle ratio euler, oracle coarse error rk4, euler, fp64 floor of the state)
    "ur10_like": (0.016, 0.002, 1.0, 16.061, 2.000, 2.72e-08, 0.0307, 6.87e-15),
    "panda_like": (0.016, 0.002, 1.0, 16.044, 1.994, 2.22e-09, 0.00426, 7.82e-16),
}


@pytest.mark.parametrize("name", ["ur10_like", "panda_like"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_order_of_the_integrators(name, integrator):
    """End-state error at dt and dt / 2 over a fixed span against an oracle RK4 rollout at dt / 8: the ratio lies in (2^3.5, 2^4.5) for RK4,
    (2^0.5, 2^1.5) for semi-implicit Euler (the geometric midpoints between neighbouring orders).  Wrong weights or a stale stage state
    cost an order."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd.samples import uniform_pm1
    chain, ref = _pair(name)
    span, dt, amp = ORDER[name][:3]
    N = 64
    q0, dq0, tau = uniform_pm1(4700, (N, ref.n)), uniform_pm1(4701, (N, ref.n)), amp * uniform_pm1(4702, (N, ref.n))
    steps = int(round(span / dt))
    qx, dqx = _np_rollout(_oracle_fd(ref), q0, dq0, tau, dt / 8, 8 * steps, "rk4")
    errs = []
    for k in (1, 2):
        q1, dq1, st = _rollout(torch, chain, q0, dq0, tau, dt / k, integrator, n_steps=k * steps)
        assert (st == 1).all()
        errs.append(max(np.abs(q1 - qx).max(), np.abs(dq1 - dqx).max()))
    ratio = errs[0] / errs[1]
    floor = EPS * max(np.abs(qx).max(), np.abs(dqx).max())
    print("%s %s: errors %.3g %.3g ratio %.3f (coarse error / fp64 floor %.3g)" % (name, integrator, errs[0], errs[1], ratio, errs[0] / floor))
    assert errs[0] >= 1e3 * floor
    lo, hi = (2 ** 3.5, 2 ** 4.5) if integrator == "rk4" else (2 ** 0.5, 2 ** 1.5)
    assert lo < ratio < hi, ratio


# ---- 6. trajectory records, plumbing
def _raw(chain, N, layout, tq, tdq, ttau, dt, integrator, T, q_end=None, dq_end=None, status=None, q_traj=None, dq_traj=None, traj_stride=0,
         every=0, tau_stride=None, chunk=0, stream=None, ws=None):
    import torch
    from rosdyn_amd._lib import INTEGRATORS as CODES, Batch, RolloutDesc, check, lib
    b = Batch()
    b.n_samples = N
    b.q, b.dq, b.ddq = tq.data_ptr(), tdq.data_ptr(), None
    b.layout = 1 if layout == "element" else 0
    b.device = -1
    b.stream = (stream or torch.cuda.current_stream()).cuda_stream
    d = RolloutDesc()
    d.n_steps, d.integrator, d.dt = T, CODES[integrator], dt
    d.tau, d.tau_step_stride = ttau.data_ptr(), (tq.numel() if tau_stride is None else tau_stride)
    ptr = lambda t: t.data_ptr() if t is not None else None
    d.q_end, d.dq_end, d.status, d.q_traj, d.dq_traj = ptr(q_end), ptr(dq_end), ptr(status), ptr(q_traj), ptr(dq_traj)
    d.traj_step_stride, d.traj_every = traj_stride, every
    nbytes = lib().rdyn_rollout_workspace_bytes(chain._h, C.byref(d), N, chunk)
    if ws is None and nbytes:
        ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    check(lib().rdyn_rollout(chain._h, C.byref(b), C.byref(d), chunk, ptr(ws), nbytes))
    return ws


@pytest.mark.parametrize("name", ["ur10_like", "ur10_public_long", "rev10", "rev14"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_trajectory_records_and_plumbing(name, integrator):
    """T = 7, traj_every 1 and 3 (7 and 2 records): record k is bitwise the end state of a rollout of (k + 1) traj_every steps; a step
    stride larger than n N with poison in the gaps, guard bands around every output, outputs on and off a 128-byte line, q_end aliasing
    batch->q, status NULL, only a trajectory requested."""
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N, T = chain.getActiveJointsNumber(), 200, 7
    q0, dq0, tau = _inputs(name, n, N, T, seed=4800)
    ends = [_rollout(torch, chain, q0, dq0, tau, DT, integrator, n_steps=k) for k in range(1, T + 1)]
    POISON, G = 12345.5, 48
    for layout in ("sample", "element"):
        ttau = _dev_seq(torch, tau, layout)
        for every, shift in ((1, 0), (3, 1), (3, 0)):
            records = T // every
            tq, tdq = _dev(torch, q0, layout), _dev(torch, dq0, layout)
            stride = n * N + (16 if shift == 0 else 5)   # 16 doubles keep the records on their lines, 5 do not
            bufs = {}
            for key, size in (("q_end", n * N), ("dq_end", n * N), ("q_traj", records * stride), ("dq_traj", records * stride)):
                big = torch.full((G + shift + size + G,), POISON, dtype=torch.float64, device="cuda")
                bufs[key] = (big, big[G + shift:G + shift + size])
                assert (bufs[key][1].data_ptr() % 128 == 0) == (shift == 0)
            sbig = torch.full((G + N + G,), 777, dtype=torch.int32, device="cuda")
            _raw(chain, N, layout, tq, tdq, ttau, DT, integrator, T, q_end=bufs["q_end"][1], dq_end=bufs["dq_end"][1], status=sbig[G:],
                 q_traj=bufs["q_traj"][1], dq_traj=bufs["dq_traj"][1], traj_stride=stride, every=every)
            torch.cuda.synchronize()
            shape = (N, n) if layout == "sample" else (n, N)
            for key, col in (("q", 0), ("dq", 1)):
                assert np.array_equal(_host(bufs[key + "_end"][1].view(shape), layout), ends[T - 1][col])
                tr = bufs[key + "_traj"][1].view(records, stride)
                for k in range(records):
                    assert np.array_equal(_host(tr[k, :n * N].view(shape), layout), ends[(k + 1) * every - 1][col]), (layout, every, key, k)
                assert (tr[:, n * N:] == POISON).all()
            for big, view in bufs.values():
                assert (big[:G + shift] == POISON).all() and (big[G + shift + view.numel():] == POISON).all()
            assert (sbig[:G] == 777).all() and (sbig[G + N:] == 777).all() and (sbig[G:G + N] == 1).all()
            assert np.array_equal(_host(tq, layout), q0) and np.array_equal(_host(ttau[0], layout), tau[0])   # the inputs are left alone
        # q_end aliasing batch->q, dq_end batch->dq; status NULL
        tq, tdq = _dev(torch, q0, layout), _dev(torch, dq0, layout)
        _raw(chain, N, layout, tq, tdq, ttau, DT, integrator, T, q_end=tq, dq_end=tdq)
        assert np.array_equal(_host(tq, layout), ends[T - 1][0]) and np.array_equal(_host(tdq, layout), ends[T - 1][1])
        # only a trajectory of q requested
        tq, tdq = _dev(torch, q0, layout), _dev(torch, dq0, layout)
        only = torch.full((2 * n * N,), POISON, dtype=torch.float64, device="cuda")
        _raw(chain, N, layout, tq, tdq, ttau, DT, integrator, T, q_traj=only, traj_stride=n * N, every=3)
        for k in range(2):
            assert np.array_equal(_host(only[k * n * N:(k + 1) * n * N].view(shape), layout), ends[3 * k + 2][0])


# ---- 7. failure is per sample and sticky
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("layout", ["sample", "element"])
def test_failure_reports_minus_one_and_nan_from_the_failing_step_on(integrator, layout):
    """ur10_public with the fixed joint of tool0 among the input joints: its row and column of M are zero."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd import Chain
    chain = Chain(os.path.join(FIXTURES, "ur10_public.urdf"), "base_link", "tool0", GRAV)
    moving = ["shoulder_pan_joint", "shoulder_lift_joint", "elbow_joint", "wrist_1_joint", "wrist_2_joint", "wrist_3_joint"]
    assert chain.setInputJointsName(moving[:3] + ["flange-tool0"] + moving[3:])
    n, N, T = 7, 200, 3
    assert chain.getActiveJointsNumber() == n
    q0, dq0, tau = _inputs("ur10_like", n, N, T, seed=4900)
    q1, dq1, st, qt, dqt = _rollout(torch, chain, q0, dq0, tau, DT, integrator, layout, trajectory_every=1)
    assert (st == -1).all() and np.isnan(q1).all() and np.isnan(dq1).all()
    assert qt.shape == (T, N, n) and np.isnan(qt).all() and np.isnan(dqt).all()
    # a valid chain in the same process afterwards still answers correctly
    good, ref = _pair("ur10_public")
    _euler_residual_check(torch, good, ref, "ur10_like", N, layout, 4901)


# ---- 8. no steps
@pytest.mark.parametrize("name", ["ur10_like", "rev14"])
@pytest.mark.parametrize("layout", ["sample", "element"])
def test_no_steps_copies_the_state(name, layout):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 200
    q0, dq0, tau = _inputs(name, n, N, 1, seed=5000)
    for integrator in INTEGRATORS:
        q1, dq1, st = _rollout(torch, chain, q0, dq0, tau, DT, integrator, layout, n_steps=0)
        assert np.array_equal(q1, q0) and np.array_equal(dq1, dq0) and (st == 1).all()


# ---- 9. graph capture
@pytest.mark.parametrize("name", ["ur10_like", "rev14"])
def test_replays_from_a_captured_graph(name):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N, T = chain.getActiveJointsNumber(), 5000, 4
    q, dq = (torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(2))
    tau = torch.rand((T, N, n), dtype=torch.float64, device="cuda") * 10 - 5
    q_end, dq_end = torch.empty_like(q), torch.empty_like(q)
    st = torch.empty((N,), dtype=torch.int32, device="cuda")
    ws = _raw(chain, N, "sample", q, dq, tau, DT, "rk4", T, q_end=q_end, dq_end=dq_end, status=st, chunk=2048)   # first use outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            _raw(chain, N, "sample", q, dq, tau, DT, "rk4", T, q_end=q_end, dq_end=dq_end, status=st, chunk=2048, stream=s, ws=ws)
    for k in range(3):
        q.uniform_(-1, 1)
        dq.uniform_(-1, 1)
        tau.uniform_(-5, 5)
        q_end.zero_()
        dq_end.zero_()
        st.zero_()
        g.replay()
        torch.cuda.synchronize()
        q2, dq2, st2 = chain.rollout(q, dq, tau, DT, integrator="rk4", chunk_samples=2048)
        assert torch.equal(q_end, q2) and torch.equal(dq_end, dq2) and torch.equal(st, st2) and bool((st == 1).all())


# ---- 10. the C++ facade
def test_facade_rollout_batch(tmp_path):
    """tests/cpp/rollout_facade.cpp: rolloutBatch on a 6-joint chain and on a generated 14-joint chain against chained
    getJointAccelerationBatch steps."""
    exe = tmp_path / "rollout_facade"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "rosdyn_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "rollout_facade.cpp"),
                           "-o", str(exe), "-L" + os.path.join(ROOT, "rosdyn_amd"), "-lrdyn_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "rosdyn_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    long_urdf = tmp_path / "rev14.urdf"
    long_urdf.write_text(generated_revolute_chain(14, 1014))
    r = subprocess.run([str(exe), os.path.join(FIXTURES, "ur10_like.urdf"), str(long_urdf)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
