"""GPU tests of the batched forward dynamics rdyn_forward_dynamics / Chain.getJointAcceleration: ddq = M(q)^-1 (tau - h(q, dq)).
The reference has no forward dynamics; the call is defined by getJointInertia (primitives_impl.h:1357-1379) and
getJointTorqueNonLinearPart (:1274-1293), which the oracle restates.

Bounds (each holds per sample, no sample is excused):
  oracle, residual form   |M_ref ddq + h_ref - tau|_inf <= 1e-11 (|M_ref|_inf |ddq|_inf + |tau|_inf + |h_ref|_inf): 1e-11 is the project's
                          parity figure for M and h; a backward-stable solve adds a few n eps.  The oracle's own numpy Cholesky solve
                          sits at <= 0.61 eps in the same ratio.
  the solver alone        M, h from the library itself, the solve redone in numpy:
                          |ddq - ddq_host|_inf <= 64 eps cond2(M) max(1, |ddq_host|_inf): Cholesky's forward error is c n eps cond2; numpy
                          LU against numpy Cholesky on oracle data: 0.43 in these units, the round trip ddq -> tau -> ddq through the
                          oracle: 5.6.
  pivots                  the smallest Cholesky pivot / trace(M) over the valid chains is >= 2e-5 (oracle), five orders above the
                          1e-10 rule: no valid sample may report -1."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import FIXTURES, ROOT
from _arrays import EPS, _dev, _host, _inf, _inputs, _solve
from _chains import CHAINS, GRAV, _chain, _pair
from _references import _solver_bound_check
from rosdyn_amd.urdf_gen import generated_revolute_chain

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("layout,N", [("sample", 4096), ("element", 4096), ("sample", 200), ("element", 200), ("sample", 1), ("element", 1)])
def test_against_the_oracle_in_residual_form(name, layout, N):
    torch = pytest.importorskip("torch")
    chain, ref = _pair(name)
    q, dq, tau = _inputs(ref.n, N)
    ddq, st = _solve(torch, chain, q, dq, tau, layout)
    assert st.shape == (N,) and (st == 1).all(), np.unique(st)
    assert np.isfinite(ddq).all()
    M = ref.joint_inertia(q)
    h = ref.joint_torque(q, dq, np.zeros_like(q))
    res = _inf(np.einsum("sij,sj->si", M, ddq) + h - tau)
    scale = np.abs(M).sum(axis=2).max(axis=1) * _inf(ddq) + _inf(tau) + _inf(h)
    print("%s %s N=%d: residual ratio max %.3g (bound 1e-11)" % (name, layout, N, (res / scale).max()))
    assert (res <= 1e-11 * scale).all(), (float((res / scale).max()), int(np.argmax(res / scale)))


@pytest.mark.parametrize("name", CHAINS)
def test_the_solver_alone_against_a_host_solve_of_the_library_own_m_and_h(name):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 4096
    q, dq, tau = _inputs(n, N, seed=501)
    ddq, st = _solve(torch, chain, q, dq, tau, "sample")
    assert (st == 1).all()
    tq, tdq = _dev(torch, q, "sample"), _dev(torch, dq, "sample")
    M = chain.getJointInertia(tq).cpu().numpy()
    h = chain.getJointTorqueNonLinearPart(tq, tdq).cpu().numpy()
    _solver_bound_check(ddq, M, h, tau, name)


@pytest.mark.parametrize("name", CHAINS)
def test_round_trip_through_the_joint_torque(name):
    torch = pytest.importorskip("torch")
    from rosdyn_amd.samples import uniform_pm1
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 4096
    q, dq, _ = _inputs(n, N, seed=901)
    ddq0 = 3.0 * uniform_pm1(905, (N, n))
    tq, tdq = _dev(torch, q, "sample"), _dev(torch, dq, "sample")
    tau = chain.getJointTorque(tq, tdq, _dev(torch, ddq0, "sample"))
    ddq, st = chain.getJointAcceleration(tq, tdq, tau)
    assert (st.cpu().numpy() == 1).all()
    cond = np.linalg.cond(chain.getJointInertia(tq).cpu().numpy())
    ratio = _inf(ddq.cpu().numpy() - ddq0) / (EPS * cond * np.maximum(1.0, _inf(ddq0)))
    print("%s: round-trip ratio max %.3g (bound 64)" % (name, ratio.max()))
    assert (ratio <= 64.0).all(), (float(ratio.max()), int(np.argmax(ratio)))


@pytest.mark.parametrize("layout", ["sample", "element"])
def test_inertia_that_is_not_positive_definite_reports_minus_one_and_nan(layout):
    """ur10_public with the fixed joint of tool0 among the input joints: its row and column of M are zero."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd import Chain
    path, base, tool = os.path.join(FIXTURES, "ur10_public.urdf"), "base_link", "tool0"
    chain = Chain(path, base, tool, GRAV)
    moving = ["shoulder_pan_joint", "shoulder_lift_joint", "elbow_joint", "wrist_1_joint", "wrist_2_joint", "wrist_3_joint"]
    assert chain.setInputJointsName(moving[:3] + ["flange-tool0"] + moving[3:])
    n, N = 7, 1000
    assert chain.getActiveJointsNumber() == n
    q, dq, tau = _inputs(n, N, seed=33)
    ddq, st = _solve(torch, chain, q, dq, tau, layout)
    assert (st == -1).all() and np.isnan(ddq).all()
    # a valid chain in the same process afterwards still answers correctly
    good, ref = _pair("ur10_public")
    q, dq, tau = _inputs(ref.n, N, seed=34)
    ddq, st = _solve(torch, good, q, dq, tau, layout)
    assert (st == 1).all()
    M, h = ref.joint_inertia(q), ref.joint_torque(q, dq, np.zeros_like(q))
    res = _inf(np.einsum("sij,sj->si", M, ddq) + h - tau)
    assert (res <= 1e-11 * (np.abs(M).sum(axis=2).max(axis=1) * _inf(ddq) + _inf(tau) + _inf(h))).all()


def _raw(chain, N, layout, tq, tdq, ttau_ptr, ddq_ptr, status_ptr, chunk=0, ws=None, stream=None):
    import torch
    from rosdyn_amd._lib import Batch, check, lib
    b = Batch()
    b.n_samples = N
    b.q, b.dq, b.ddq = tq.data_ptr(), tdq.data_ptr(), None
    b.layout = 1 if layout == "element" else 0
    b.device = -1
    b.stream = (stream or torch.cuda.current_stream()).cuda_stream
    check(lib().rdyn_forward_dynamics(chain._h, C.byref(b), ttau_ptr, ddq_ptr, status_ptr, chunk, ws.data_ptr() if ws is not None else None,
                                      ws.numel() if ws is not None else 0))


@pytest.mark.parametrize("name", ["ur10_like", "panda_like", "ur10_public_long", "rev10", "rev14", "gen20_permuted"])
def test_plumbing_alias_null_status_unaligned_output_guard_bands_and_layouts(name):
    torch = pytest.importorskip("torch")
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 1000
    q, dq, tau = _inputs(n, N, seed=11)
    ref_ddq, ref_st = _solve(torch, chain, q, dq, tau, "sample")
    assert (ref_st == 1).all()
    # element-major equals sample-major bitwise
    el_ddq, el_st = _solve(torch, chain, q, dq, tau, "element")
    assert np.array_equal(el_ddq, ref_ddq) and np.array_equal(el_st, ref_st)
    nbytes = lib().rdyn_forward_dynamics_workspace_bytes(chain._h, 0)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda") if nbytes else None
    for layout in ("sample", "element"):
        tq, tdq = _dev(torch, q, layout), _dev(torch, dq, layout)
        # ddq aliasing tau, status NULL
        buf = _dev(torch, tau, layout)
        _raw(chain, N, layout, tq, tdq, buf.data_ptr(), buf.data_ptr(), None, ws=ws)
        assert np.array_equal(_host(buf, layout), ref_ddq)
        # an output that does not start on a 128-byte line, guard bands around ddq and status
        G = 24
        big = torch.full((G + 1 + N * n + G,), 12345.5, dtype=torch.float64, device="cuda")
        sbig = torch.full((G + N + G,), 777, dtype=torch.int32, device="cuda")
        out = big[G + 1:G + 1 + N * n]
        assert out.data_ptr() % 128 != 0
        ttau = _dev(torch, tau, layout)
        _raw(chain, N, layout, tq, tdq, ttau.data_ptr(), out.data_ptr(), sbig[G:].data_ptr(), ws=ws)
        torch.cuda.synchronize()
        got = out.view((N, n) if layout == "sample" else (n, N))
        assert np.array_equal(_host(got, layout), ref_ddq)
        assert (big[:G + 1] == 12345.5).all() and (big[G + 1 + N * n:] == 12345.5).all()
        assert (sbig[:G] == 777).all() and (sbig[G + N:] == 777).all() and (sbig[G:G + N] == 1).all()
        assert np.array_equal(_host(ttau, layout), tau)   # the torques are left alone when ddq does not alias them


def test_chunk_size_does_not_change_the_result():
    torch = pytest.importorskip("torch")
    chain = _chain("rev20")
    n, N = 20, 40000
    q, dq, tau = _inputs(n, N, seed=21)
    a, sa = _solve(torch, chain, q, dq, tau, "sample", chunk_samples=16384)
    b, sb = _solve(torch, chain, q, dq, tau, "sample", chunk_samples=(N + 2) // 3)
    c, sc = _solve(torch, chain, q, dq, tau, "element", chunk_samples=1000)
    assert np.array_equal(a, b) and np.array_equal(a, c) and (sa == 1).all() and (sb == 1).all() and (sc == 1).all()


@pytest.mark.parametrize("name", ["ur10_like", "rev14"])
def test_replays_from_a_captured_graph(name):
    torch = pytest.importorskip("torch")
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 20000
    q, dq, tau = (torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(3))
    ddq = torch.empty_like(q)
    st = torch.empty((N,), dtype=torch.int32, device="cuda")
    nbytes = lib().rdyn_forward_dynamics_workspace_bytes(chain._h, 8192)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda") if nbytes else None
    _raw(chain, N, "sample", q, dq, tau.data_ptr(), ddq.data_ptr(), st.data_ptr(), chunk=8192, ws=ws)   # first use outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            _raw(chain, N, "sample", q, dq, tau.data_ptr(), ddq.data_ptr(), st.data_ptr(), chunk=8192, ws=ws, stream=s)
    for k in range(3):
        q.uniform_(-1, 1)
        dq.uniform_(-1, 1)
        tau.uniform_(-50, 50)
        ddq.zero_()
        st.zero_()
        g.replay()
        torch.cuda.synchronize()
        ddq2, st2 = chain.getJointAcceleration(q, dq, tau, chunk_samples=8192)
        assert torch.equal(ddq, ddq2) and torch.equal(st, st2) and bool((st == 1).all())


def test_facade_batch_method_and_single_sample_getter(tmp_path):
    """tests/cpp/forward_dynamics_facade.cpp: getJointAccelerationBatch and getJointAcceleration of the C++ facade (6 joints in
    registers, 14 input joints through the chunked route, the exception on a fixed input joint)."""
    exe = tmp_path / "fwd_facade"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "rosdyn_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "forward_dynamics_facade.cpp"),
                           "-o", str(exe), "-L" + os.path.join(ROOT, "rosdyn_amd"), "-lrdyn_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "rosdyn_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    long_urdf = tmp_path / "rev14.urdf"
    long_urdf.write_text(generated_revolute_chain(14, 1014))
    r = subprocess.run([str(exe), os.path.join(FIXTURES, "ur10_like.urdf"), os.path.join(FIXTURES, "ur10_public.urdf"), str(long_urdf)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
