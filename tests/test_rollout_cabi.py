"""CPU tests (no GPU): argument checks and the workspace query of rdyn_rollout (include/rdyn.h).
Nothing here touches a device: every call either has no samples or fails its checks first."""
import ctypes as C

import pytest

from _cabi import CHUNKED, EULER, FAKE, RDYN_ERR_INVALID_ARGUMENT, RDYN_OK, RK4, SWEPT, _chain, _query, _rollout_desc as _desc


def _call(chain, N, desc=True, chunk_samples=0, workspace=FAKE, workspace_bytes=None, q=FAKE, dq=FAKE, batch=True, layout=0, **kw):
    from rosdyn_amd._lib import Batch, lib
    b = Batch()
    b.n_samples, b.q, b.dq, b.layout, b.device = N, q, dq, layout, 0
    d = _desc(chain.getActiveJointsNumber(), max(N, 0), **kw)
    if workspace_bytes is None:
        workspace_bytes = _query(chain, d, max(N, 0), max(chunk_samples, 0))
    return lib().rdyn_rollout(chain._h, C.byref(b) if batch else None, C.byref(d) if desc else None, chunk_samples, workspace, workspace_bytes)


@pytest.mark.parametrize("name", SWEPT + CHUNKED)
def test_no_samples_is_ok_and_every_listed_refusal(name):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 7
    assert _call(chain, 0) == RDYN_OK
    assert _call(chain, 0, q=None, dq=None, q_end=None, dq_end=None, status=None, workspace=None, workspace_bytes=0) == RDYN_OK
    assert _call(chain, 0, layout=1, integrator=EULER) == RDYN_OK
    refusals = [
        {"desc": False},                                        # null desc
        {"tau": None},                                          # null tau with T > 0
        {"q_end": None, "dq_end": None},                        # all four outputs null with N > 0
        {"n_steps": -1},
        {"dt": 0.0}, {"dt": float("inf")}, {"dt": float("-inf")}, {"dt": float("nan")},
        {"integrator": 2}, {"integrator": -1},
        {"q_traj": FAKE, "traj_every": 0, "traj_step_stride": n * N},
        {"dq_traj": FAKE, "traj_every": -3, "traj_step_stride": n * N},
        {"q_traj": FAKE, "traj_every": 1, "traj_step_stride": n * N - 1},
        {"dq_traj": FAKE, "traj_every": 2, "traj_step_stride": 0},
        {"chunk_samples": -1},
        {"q": None}, {"dq": None}, {"batch": False},
    ]
    for kw in refusals:
        assert _call(chain, N, **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
        assert lib().rdyn_last_error()
    assert _call(chain, -1) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, N, layout=5) == RDYN_ERR_INVALID_ARGUMENT
    # refusals do not depend on there being samples, except the one that says so
    assert _call(chain, 0, desc=False) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 0, dt=0.0) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 0, chunk_samples=-1) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 0, q_end=None, dq_end=None) == RDYN_OK
    # a null torque pointer is fine when no step is taken
    assert _call(chain, 0, tau=None, n_steps=0) == RDYN_OK
    assert lib().rdyn_rollout(None, None, None, 0, FAKE, 1 << 30) == RDYN_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", SWEPT + ["rev10"])
def test_register_route_needs_no_workspace(name):
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    assert n <= 10
    for integrator in (EULER, RK4):
        for N in (0, 1, 4096, 1 << 20):
            for chunk in (0, 1, 16384):
                assert _query(chain, _desc(n, N, integrator=integrator), N, chunk) == 0


@pytest.mark.parametrize("name", CHUNKED)
@pytest.mark.parametrize("integrator", [EULER, RK4])
def test_workspace_of_the_chunked_route(name, integrator):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 5000
    assert n > 10
    d = _desc(n, N, integrator=integrator)
    chunks = (1, 64, 1000, 16384, 100000)
    sizes = [_query(chain, d, N, chunk) for chunk in chunks]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
    arrays = 7 if integrator == RK4 else 3
    for chunk, s in zip(chunks + (0,), sizes + [_query(chain, d, N, 0)]):
        fd = lib().rdyn_forward_dynamics_workspace_bytes(chain._h, chunk)
        assert s >= fd + arrays * n * N * 8 and s >= fd
    assert _query(chain, d, 2 * N, 1000) > _query(chain, d, N, 1000)
    assert _query(chain, d, N, -5) == 0
    # an undersized or missing workspace is refused before any device work
    need = _query(chain, d, 7, 1000)
    assert _call(chain, 7, integrator=integrator, chunk_samples=1000, workspace_bytes=need - 1) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 7, integrator=integrator, chunk_samples=1000, workspace=None, workspace_bytes=need) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 7, integrator=integrator, workspace_bytes=0) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 0, integrator=integrator, workspace=None, workspace_bytes=0) == RDYN_OK


def test_python_binding_exists():
    from rosdyn_amd import Chain
    assert callable(getattr(Chain, "rollout"))
