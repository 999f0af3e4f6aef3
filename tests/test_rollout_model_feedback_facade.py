"""The model-based laws through the C++ facade (rosdyn_chain_facade.hpp: the rolloutWorkspaceBytes / rolloutBatch overloads that take a
rdyn_feedback and a rdyn_model_feedback): tests/cpp/rollout_model_feedback_facade.cpp builds pedantic against the stand-in Eigen headers
(CPU), and on the GPU gives the Python binding's own bits."""
import os
import subprocess

import numpy as np
import pytest

from conftest import FIXTURES, ROOT
from _arrays import _value
from _chains import FACADE_CHAINS
from _model_feedback import _model


def _build(tmp_path):
    exe = tmp_path / "rollout_model_feedback_facade"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "tests", "mock_include"), "-I" + os.path.join(ROOT, "rosdyn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "rollout_model_feedback_facade.cpp"), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "rosdyn_amd"), "-lrdyn_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "rosdyn_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def test_the_facade_caller_builds_pedantic_against_the_stand_in_eigen_headers(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("urdf,base,tool", FACADE_CHAINS)
def test_the_facade_gives_the_python_binding_own_bits(tmp_path, urdf, base, tool):
    torch = pytest.importorskip("torch")
    from rosdyn_amd import Chain, ModelFeedback
    exe = _build(tmp_path)
    r = subprocess.run([exe, os.path.join(FIXTURES, urdf), base, tool], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout + r.stderr
    got = {ln.split()[0]: np.array([float(x) for x in ln.split()[1:]]) for ln in r.stdout.splitlines() if " " in ln}
    chain = Chain(os.path.join(FIXTURES, urdf), base, tool, (0.0, 0.0, -9.806))
    model = _model(chain)
    n, N, T = chain.getActiveJointsNumber(), 5, 3
    grid = lambda k, m=n: np.array([[_value(s, i, k) for i in range(m)] for s in range(N)])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    q, dq = dev(grid(0)), dev(grid(1))
    tau = dev(np.stack([0.5 * grid(2 + t) for t in range(T)]))
    q_ref, dq_ref, ddq_ref = (dev(np.stack([grid(k + t) for t in range(T)])) for k in (20, 30, 40))
    kp, kd, lim = dev(4.0 + np.arange(n)), dev(0.5 + 0.25 * np.arange(n)), dev(np.full(n, 2.0))
    w_tool = dev(0.5 * grid(12, 6))
    fb = ModelFeedback(model, "computed_torque", q_ref, kp, kd, dq_ref, ddq_ref, hold=True, tau_limit=lim, command_trajectory=True)
    q1, dq1, st, _, _, ut = chain.rollout(q, dq, tau, 1e-3, integrator="rk4", trajectory_every=1, feedback=fb)
    assert bool((st == 1).all())
    assert np.array_equal(got["q_end"], q1.cpu().numpy().ravel()) and np.array_equal(got["dq_end"], dq1.cpu().numpy().ravel())
    assert np.array_equal(got["u_last"], ut[T - 1].cpu().numpy().ravel())
    fb = ModelFeedback(model, "gravity_compensation", q_ref, kp, kd, dq_ref, hold=False, tau_limit=lim)
    q2, dq2, st = chain.rollout(q, dq, tau, 1e-3, integrator="rk4", feedback=fb, ext_wrenches=w_tool, ext_link=chain.getLinksName()[-1])
    assert bool((st == 1).all())
    assert np.array_equal(got["q_end_tool"], q2.cpu().numpy().ravel()) and np.array_equal(got["dq_end_tool"], dq2.cpu().numpy().ravel())
    assert not np.array_equal(got["q_end_tool"], got["q_end"])
