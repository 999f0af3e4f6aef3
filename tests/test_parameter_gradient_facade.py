"""The parameter gradients of the C++ facade (rosdyn_chain_facade.hpp: withParameters, getJointAccelerationParameterVjpBatch,
rolloutParameterAdjointBatch and their workspace queries) through tests/cpp/parameter_gradient_facade.cpp: it builds host-only, pedantic,
against the stand-in Eigen headers, and on the GPU its results are the Python binding's bits."""
import os
import subprocess

import numpy as np
import pytest

from conftest import FIXTURES, ROOT

CHAINS = [("ur10_like.urdf", "base_link", "tool0"), ("mixed_joints.urdf", "world", "tip")]


def _build(tmp_path):
    exe = tmp_path / "parameter_gradient_facade"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "tests", "mock_include"), "-I" + os.path.join(ROOT, "rosdyn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "parameter_gradient_facade.cpp"), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "rosdyn_amd"), "-lrdyn_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "rosdyn_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def test_the_caller_builds_pedantic_against_the_stand_in_eigen_headers(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def _value(s, i, k):
    return ((s * 7 + i * 3 + k * 5) % 17 - 8) / 16.0


@pytest.mark.gpu
@pytest.mark.parametrize("urdf,base,tool", CHAINS)
def test_the_facade_gives_the_python_binding_own_bits(tmp_path, urdf, base, tool):
    torch = pytest.importorskip("torch")
    from rosdyn_amd import Chain
    from rosdyn_amd.components import ComponentSet
    exe = _build(tmp_path)
    r = subprocess.run([exe, os.path.join(FIXTURES, urdf), base, tool], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout + r.stderr
    got = {ln.split()[0]: np.array([float(x) for x in ln.split()[1:]]) for ln in r.stdout.splitlines() if " " in ln}
    nominal = Chain(os.path.join(FIXTURES, urdf), base, tool, (0.0, 0.0, -9.806))
    pi0 = nominal.getNominalParameters()
    chain = nominal.withParameters(pi0 * (1.0 + ((np.arange(pi0.size) * 5) % 9 - 4) / 64.0))
    n, N, T = chain.getActiveJointsNumber(), 5, 3
    cs = ComponentSet([dict(type=0, joint=0, min_velocity=0.0625, max_velocity=0.75, parameters=[0.25, 0.5, 0.0]),
                       dict(type=2, joint=n - 1, min_velocity=0.0, max_velocity=0.0, parameters=[1.5, -0.25, 0.0])], n)
    grid = lambda k: np.array([[_value(s, i, k) for i in range(n)] for s in range(N)])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    q, dq, gq, gv = dev(grid(0)), dev(grid(1)), dev(grid(9)), dev(grid(10))
    tau = dev(np.stack([0.5 * grid(2 + t) for t in range(T)]))
    fw = chain.rollout(q, dq, tau, 1e-3, integrator="rk4", trajectory_every=1, components=cs)
    assert bool((fw[2] == 1).all())
    adj = chain.rolloutParameterAdjoint(q, dq, tau, 1e-3, fw[3], fw[4], gq_end=gq, gDq_end=gv, integrator="rk4", components=cs)
    assert bool((adj[5] == 1).all())
    for key, t in zip(("gq0", "gdq0", "gtau", "gpi", "gcomp"), adj[:5]):
        assert np.array_equal(got[key], t.cpu().numpy().ravel()), key
    rows = chain.getJointAccelerationParameterVjp(q, dq, tau[0], gq, components=cs)
    for key, t in zip(("pi_bar", "comp_bar", "tau_bar", "ddq"), rows[:4]):
        assert np.array_equal(got[key], t.cpu().numpy().ravel()), key
    sums = chain.getJointAccelerationParameterVjp(q, dq, tau[0], gq, components=cs, reduce=True)
    assert np.array_equal(got["pi_bar_sum"], sums[0].cpu().numpy()) and np.array_equal(got["comp_bar_sum"], sums[1].cpu().numpy())
