"""The parameter gradients of the closed loop through the C++ facade (rosdyn_chain_facade.hpp: the rolloutParameterAdjointBatch /
rolloutParameterAdjointWorkspaceBytes overloads with a rdyn_feedback and a rdyn_feedback_gradient pointer) through
tests/cpp/rollout_feedback_parameter_adjoint_facade.cpp: it builds host-only, pedantic, against the stand-in Eigen headers, and on the GPU
its results are the Python binding's bits."""
import os
import subprocess

import numpy as np
import pytest

from conftest import FIXTURES, ROOT
from _arrays import _value
from _chains import FACADE_CHAINS as CHAINS


def _build(tmp_path):
    exe = tmp_path / "rollout_feedback_parameter_adjoint_facade"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "tests", "mock_include"), "-I" + os.path.join(ROOT, "rosdyn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "rollout_feedback_parameter_adjoint_facade.cpp"), "-o", str(exe),
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
    from rosdyn_amd import Chain, Feedback
    exe = _build(tmp_path)
    r = subprocess.run([exe, os.path.join(FIXTURES, urdf), base, tool], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout + r.stderr
    got = {ln.split()[0]: np.array([float(x) for x in ln.split()[1:]]) for ln in r.stdout.splitlines() if " " in ln}
    chain = Chain(os.path.join(FIXTURES, urdf), base, tool, (0.0, 0.0, -9.806))
    n, N, T = chain.getActiveJointsNumber(), 5, 3
    grid = lambda k, m=n: np.array([[_value(s, i, k) for i in range(m)] for s in range(N)])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    flat = lambda t: t.cpu().numpy().ravel()
    q, dq, seed = dev(grid(0)), dev(grid(1)), dev(grid(9))
    tau = dev(np.stack([0.5 * grid(2 + t) for t in range(T)]))
    q_ref = dev(np.stack([grid(0) + 0.25 * grid(20 + t) for t in range(T)]))
    dq_ref = dev(np.stack([grid(1) + 0.25 * grid(24 + t) for t in range(T)]))
    gu = dev(np.stack([grid(28 + t) for t in range(T)]))
    fb = Feedback(q_ref, dev(2.0 + 0.25 * np.arange(n)), dev(0.5 + 0.125 * np.arange(n)), dq_ref, hold=True, tau_limit=dev(np.full(n, 0.75)))
    names = ("q_ref", "Dq_ref", "kp", "kd", "tau_limit")
    fw = chain.rollout(q, dq, tau, 1e-3, integrator="rk4", trajectory_every=1, feedback=fb)
    assert bool((fw[2] == 1).all())
    g = chain.rolloutParameterAdjoint(q, dq, tau, 1e-3, fw[3], fw[4], gq_end=seed, integrator="rk4", feedback=fb, want_feedback=names, gu_traj=gu)
    assert bool((g[5] == 1).all()) and g[4] is None
    keys = ("gq0", "gdq0", "gtau", "gpi", None, None, "gq_ref", "gdq_ref", "gkp", "gkd", "glim")
    for key, t in zip(keys, g):
        if key:
            assert np.array_equal(got[key], flat(t)), key
    # with a null rdyn_feedback_gradient the law's outputs are left alone (the program's buffers still hold the first call's) and gpi, gq0,
    # gdq0, gtau are the same bits: gu_traj is part of the gradient selection, so the bare call has no seeds on the command record
    bare = chain.rolloutParameterAdjoint(q, dq, tau, 1e-3, fw[3], fw[4], gq_end=seed, integrator="rk4", feedback=fb)
    for key, t in zip(("gq0_bare", "gdq0_bare", "gtau_bare", "gpi_bare"), bare):
        assert np.array_equal(got[key], flat(t)), key
    assert np.array_equal(got["gkp_bare"], got["gkp"]) and not np.array_equal(got["gpi_bare"], got["gpi"])
    assert np.abs(got["gpi"]).max() > 0 and np.abs(got["glim"]).max() > 0 and (got["glim"] == 0.0).any()
