"""The external-wrench calls of the C++ facade (rosdyn_chain_facade.hpp: getJointAcceleration(q, Dq, tau, ext_wrenches_in_link_frame),
getJointAccelerationBatch / rolloutBatch with a rdyn_ext_wrenches and their workspace queries) through
tests/cpp/forward_dynamics_ext_facade.cpp: it builds host-only, pedantic, against the stand-in Eigen headers, and on the GPU its results are
the Python binding's bits."""
import os
import subprocess

import numpy as np
import pytest

from conftest import FIXTURES, ROOT
from _arrays import _value
from _chains import FACADE_CHAINS as CHAINS


def _build(tmp_path):
    exe = tmp_path / "forward_dynamics_ext_facade"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "tests", "mock_include"), "-I" + os.path.join(ROOT, "rosdyn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "forward_dynamics_ext_facade.cpp"), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "rosdyn_amd"), "-lrdyn_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "rosdyn_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def test_the_caller_builds_pedantic_against_the_stand_in_eigen_headers(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("urdf,base,tool", CHAINS)
def test_the_facade_gives_the_python_binding_own_bits(tmp_path, urdf, base, tool):
    torch = pytest.importorskip("torch")
    from rosdyn_amd import Chain
    exe = _build(tmp_path)
    r = subprocess.run([exe, os.path.join(FIXTURES, urdf), base, tool], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout + r.stderr
    got = {ln.split()[0]: np.array([float(x) for x in ln.split()[1:]]) for ln in r.stdout.splitlines() if " " in ln}
    chain = Chain(os.path.join(FIXTURES, urdf), base, tool, (0.0, 0.0, -9.806))
    n, L, N, T = chain.getActiveJointsNumber(), chain.getLinksNumber(), 5, 3
    grid = lambda k, m=n: np.array([[_value(s, i, k) for i in range(m)] for s in range(N)])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    q, dq = dev(grid(0)), dev(grid(1))
    tau = dev(np.stack([0.5 * grid(2 + t) for t in range(T)]))
    w_all = dev(0.25 * grid(11, 6 * L).reshape(N, L, 6))
    w_tool = dev(np.stack([0.5 * grid(12 + t, 6) for t in range(T)]))
    ddq, st = chain.getJointAcceleration(q, dq, tau[0], ext_wrenches=w_all)
    assert bool((st == 1).all())
    assert np.array_equal(got["ddq"], ddq.cpu().numpy().ravel())
    assert np.array_equal(got["single"], ddq[0].cpu().numpy())
    q1, dq1, st = chain.rollout(q, dq, tau, 1e-3, integrator="rk4", ext_wrenches=w_all)
    assert bool((st == 1).all())
    assert np.array_equal(got["q_end"], q1.cpu().numpy().ravel()) and np.array_equal(got["dq_end"], dq1.cpu().numpy().ravel())
    q2, dq2, st = chain.rollout(q, dq, tau, 1e-3, integrator="rk4", ext_wrenches=w_tool, ext_link=chain.getLinksName()[-1])
    assert bool((st == 1).all())
    assert np.array_equal(got["q_end_tool"], q2.cpu().numpy().ravel()) and np.array_equal(got["dq_end_tool"], dq2.cpu().numpy().ravel())
    assert not np.array_equal(got["q_end_tool"], got["q_end"])
