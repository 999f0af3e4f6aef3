"""CPU tests (no GPU): the five workspace queries of the forward-dynamics family, pinned byte for byte to the values recorded in
tests/golden/dynamics_workspace_bytes.json (tools/record_dynamics_workspace_bytes.py wrote it; it is recorded once and not
regenerated from the build under test), and the nesting the layouts promise.  A workspace a caller sized with an earlier build
must still fit.  Nothing here touches a device."""
import ctypes as C
import json
import os

import pytest

from conftest import GOLDEN
from test_forward_dynamics_cabi import CHUNKED, SWEPT, _chain

GOLDEN_FILE = os.path.join(GOLDEN, "dynamics_workspace_bytes.json")
CHUNKS = (0, 1, 64, 1000, 16384)
SAMPLES = (0, 1, 4096)
INTEGRATORS = (0, 1)   # semi-implicit Euler, RK4
FAKE = 4096


def _rollout_desc(integrator):
    from rosdyn_amd._lib import RolloutDesc
    d = RolloutDesc()
    d.n_steps, d.integrator, d.dt, d.tau, d.q_end = 5, integrator, 1e-3, FAKE, FAKE
    return d


def _adjoint_desc(integrator):
    from rosdyn_amd._lib import RolloutAdjointDesc
    d = RolloutAdjointDesc()
    d.n_steps, d.integrator, d.dt, d.tau, d.gq0 = 5, integrator, 1e-3, FAKE, FAKE
    return d


def measure(name):
    """Every pinned query of one chain: {query: {key: bytes}}; key = "chunk" or "integrator/n_samples/chunk"."""
    from rosdyn_amd._lib import lib
    chain = _chain(name)   # (kept alive while its handle is in use)
    l, h = lib(), chain._h
    out = {"forward": {}, "derivatives": {}, "vjp": {}, "rollout": {}, "adjoint": {}}
    for chunk in CHUNKS:
        out["forward"][str(chunk)] = l.rdyn_forward_dynamics_workspace_bytes(h, chunk)
        out["derivatives"][str(chunk)] = l.rdyn_forward_dynamics_derivatives_workspace_bytes(h, chunk)
        out["vjp"][str(chunk)] = l.rdyn_forward_dynamics_vjp_workspace_bytes(h, chunk)
        for integrator in INTEGRATORS:
            rd, ad = _rollout_desc(integrator), _adjoint_desc(integrator)
            for N in SAMPLES:
                key = "%d/%d/%d" % (integrator, N, chunk)
                out["rollout"][key] = l.rdyn_rollout_workspace_bytes(h, C.byref(rd), N, chunk)
                out["adjoint"][key] = l.rdyn_rollout_adjoint_workspace_bytes(h, C.byref(ad), N, chunk)
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", CHUNKED)
def test_queries_return_the_recorded_bytes(name, golden):
    got = measure(name)
    assert sorted(got) == sorted(golden[name])
    for query, sizes in got.items():
        assert len(sizes) == (len(CHUNKS) if query in ("forward", "derivatives", "vjp") else len(CHUNKS) * len(SAMPLES) * len(INTEGRATORS))
        assert sizes == golden[name][query], query
        assert all(s > 0 and s % 256 == 0 for s in sizes.values()), query


@pytest.mark.parametrize("name", CHUNKED)
def test_layouts_nest(name):
    got = measure(name)
    for chunk in CHUNKS:
        k = str(chunk)
        assert got["derivatives"][k] >= got["forward"][k]
        assert got["vjp"][k] >= got["derivatives"][k]
        for integrator in INTEGRATORS:
            for N in SAMPLES:
                key = "%d/%d/%d" % (integrator, N, chunk)
                assert got["adjoint"][key] >= got["vjp"][k]
                assert got["rollout"][key] >= got["forward"][k]


@pytest.mark.parametrize("name", SWEPT)
def test_swept_chains_need_none(name):
    for sizes in measure(name).values():
        assert all(s == 0 for s in sizes.values())
