"""CPU tests (no GPU): argument checks and the workspace queries of rdyn_forward_dynamics_vjp and rdyn_rollout_adjoint
(include/rdyn.h).  Nothing here touches a device: every call either has no samples or fails its checks first."""
import ctypes as C

import pytest

from _cabi import CHUNKED, EULER, FAKE, RDYN_ERR_INVALID_ARGUMENT, RDYN_OK, RK4, SWEPT, _adj_query, _adjoint_desc as _desc, _chain, _comp, _vjp_query


# ---- rdyn_forward_dynamics_vjp ------------------------------------------------------------------------------------


def _vjp(chain, N, q=FAKE, dq=FAKE, tau=FAKE, seed=FAKE, q_bar=FAKE, dq_bar=FAKE, tau_bar=FAKE, ddq=FAKE, status=FAKE, comps=None, n_comps=0,
         chunk_samples=0, workspace=FAKE, workspace_bytes=None, batch=True, layout=0):
    from rosdyn_amd._lib import Batch, lib
    b = Batch()
    b.n_samples, b.q, b.dq, b.layout, b.device = N, q, dq, layout, 0
    if workspace_bytes is None:
        workspace_bytes = _vjp_query(chain, max(chunk_samples, 0))
    return lib().rdyn_forward_dynamics_vjp(chain._h, C.byref(b) if batch else None, comps, n_comps, tau, seed, q_bar, dq_bar, tau_bar, ddq, status,
                                           chunk_samples, workspace, workspace_bytes)


@pytest.mark.parametrize("name", SWEPT + CHUNKED)
def test_vjp_no_samples_is_ok_and_every_listed_refusal(name):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    assert _vjp(chain, 0) == RDYN_OK
    assert _vjp(chain, 0, q=None, dq=None, tau=None, seed=None, q_bar=None, dq_bar=None, tau_bar=None, ddq=None, status=None, workspace=None,
                workspace_bytes=0) == RDYN_OK
    assert _vjp(chain, 0, layout=1) == RDYN_OK
    one = _comp()
    bad_type, bad_joint = _comp(ctype=77), _comp(joint=n)
    refusals = [
        {"q": None}, {"dq": None}, {"batch": False},
        {"tau": None}, {"seed": None},
        {"q_bar": None, "dq_bar": None, "tau_bar": None},
        {"chunk_samples": -1},
        {"comps": None, "n_comps": 1}, {"comps": C.addressof(one), "n_comps": -1}, {"comps": C.addressof(one), "n_comps": 31},
        {"comps": C.addressof(bad_type), "n_comps": 1}, {"comps": C.addressof(bad_joint), "n_comps": 1},
    ]
    for kw in refusals:
        assert _vjp(chain, 7, **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
        assert lib().rdyn_last_error()
    assert _vjp(chain, -1) == RDYN_ERR_INVALID_ARGUMENT
    assert _vjp(chain, 7, layout=5) == RDYN_ERR_INVALID_ARGUMENT
    assert _vjp(chain, 0, chunk_samples=-1) == RDYN_ERR_INVALID_ARGUMENT
    assert _vjp(chain, 0, comps=None, n_comps=1) == RDYN_ERR_INVALID_ARGUMENT
    # the optional outputs are optional: nothing is refused for a null ddq, status or any two of the three products
    assert _vjp(chain, 0, ddq=None, status=None, q_bar=None, dq_bar=None) == RDYN_OK
    assert lib().rdyn_forward_dynamics_vjp(None, None, None, 0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0, FAKE, 1 << 30) == RDYN_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", SWEPT + ["rev10"])
def test_register_routes_need_no_workspace(name):
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    assert n <= 10
    for chunk in (0, 1, 16384, 1 << 20):
        assert _vjp_query(chain, chunk) == 0
        for integrator in (EULER, RK4):
            for N in (0, 1, 4096, 1 << 20):
                assert _adj_query(chain, _desc(n, N, integrator=integrator), N, chunk) == 0


@pytest.mark.parametrize("name", CHUNKED)
def test_vjp_workspace_of_the_chunked_route(name):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    assert n > 10
    chunks = (1, 64, 1000, 16384, 100000)
    sizes = [_vjp_query(chain, chunk) for chunk in chunks]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
    for chunk, s in zip(chunks, sizes):
        # the derivative call's own workspace, three matrices and the seeds of one chunk
        assert s >= lib().rdyn_forward_dynamics_derivatives_workspace_bytes(chain._h, chunk) + chunk * (3 * n * n + n) * 8
    assert _vjp_query(chain, -5) == 0
    need = _vjp_query(chain, 1000)
    assert _vjp(chain, 7, chunk_samples=1000, workspace_bytes=need - 1) == RDYN_ERR_INVALID_ARGUMENT
    assert _vjp(chain, 7, chunk_samples=1000, workspace=None, workspace_bytes=need) == RDYN_ERR_INVALID_ARGUMENT
    assert _vjp(chain, 7, workspace_bytes=0) == RDYN_ERR_INVALID_ARGUMENT
    assert _vjp(chain, 0, workspace=None, workspace_bytes=0) == RDYN_OK


# ---- rdyn_rollout_adjoint -----------------------------------------------------------------------------------------


def _adj(chain, N, desc=True, comps=None, n_comps=0, chunk_samples=0, workspace=FAKE, workspace_bytes=None, q=FAKE, dq=FAKE, batch=True, layout=0,
         **kw):
    from rosdyn_amd._lib import Batch, lib
    b = Batch()
    b.n_samples, b.q, b.dq, b.layout, b.device = N, q, dq, layout, 0
    d = _desc(chain.getActiveJointsNumber(), max(N, 0), **kw)
    if workspace_bytes is None:
        workspace_bytes = _adj_query(chain, d, max(N, 0), max(chunk_samples, 0))
    return lib().rdyn_rollout_adjoint(chain._h, C.byref(b) if batch else None, C.byref(d) if desc else None, comps, n_comps, chunk_samples,
                                      workspace, workspace_bytes)


@pytest.mark.parametrize("name", SWEPT + CHUNKED)
def test_adjoint_no_samples_is_ok_and_every_listed_refusal(name):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 7
    assert _adj(chain, 0) == RDYN_OK
    assert _adj(chain, 0, q=None, dq=None, gq0=None, gdq0=None, gtau=None, status=None, gq_end=None, gdq_end=None, gq_traj=None, gdq_traj=None,
                workspace=None, workspace_bytes=0) == RDYN_OK
    assert _adj(chain, 0, layout=1, integrator=EULER) == RDYN_OK
    one = _comp()
    bad_type, bad_joint = _comp(ctype=77), _comp(joint=n)
    refusals = [
        {"desc": False},                                        # a null descriptor
        {"n_steps": -1},                                        # the forward call's errors
        {"dt": 0.0}, {"dt": float("inf")}, {"dt": float("-inf")}, {"dt": float("nan")},
        {"integrator": 2}, {"integrator": -1},
        {"tau": None},
        {"q_traj": None}, {"dq_traj": None}, {"q_traj": None, "n_steps": 2},   # a null trajectory pointer with T >= 2
        {"traj_step_stride": n * N - 1}, {"traj_step_stride": 0},
        {"gtraj_step_stride": n * N - 1}, {"gtraj_step_stride": 0, "gq_traj": None},
        {"gtau_step_stride": n * N - 1}, {"gtau_step_stride": 1}, {"gtau_step_stride": -n * N},
        {"gq0": None, "gdq0": None, "gtau": None},             # every output null with samples
        {"comps": None, "n_comps": 1}, {"comps": C.addressof(one), "n_comps": -1}, {"comps": C.addressof(one), "n_comps": 31},
        {"comps": C.addressof(bad_type), "n_comps": 1}, {"comps": C.addressof(bad_joint), "n_comps": 1},
        {"chunk_samples": -1},
        {"q": None}, {"dq": None}, {"batch": False},
    ]
    for kw in refusals:
        assert _adj(chain, N, **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
        assert lib().rdyn_last_error()
    assert _adj(chain, -1) == RDYN_ERR_INVALID_ARGUMENT
    assert _adj(chain, N, layout=5) == RDYN_ERR_INVALID_ARGUMENT
    # refusals do not depend on there being samples, except the one that says so
    assert _adj(chain, 0, desc=False) == RDYN_ERR_INVALID_ARGUMENT
    assert _adj(chain, 0, dt=0.0) == RDYN_ERR_INVALID_ARGUMENT
    assert _adj(chain, 0, chunk_samples=-1) == RDYN_ERR_INVALID_ARGUMENT
    assert _adj(chain, 0, q_traj=None) == RDYN_ERR_INVALID_ARGUMENT
    assert _adj(chain, 0, gq0=None, gdq0=None, gtau=None) == RDYN_OK
    # what is optional is optional: one step reads no trajectory, no step needs no torques, the sum over the steps is stride 0
    assert _adj(chain, 0, n_steps=1, q_traj=None, dq_traj=None, traj_step_stride=0) == RDYN_OK
    assert _adj(chain, 0, n_steps=0, tau=None, q_traj=None, dq_traj=None) == RDYN_OK
    assert _adj(chain, 0, gtau_step_stride=0) == RDYN_OK
    assert _adj(chain, 0, gq_end=None, gdq_end=None, gq_traj=None, gdq_traj=None, gtraj_step_stride=0) == RDYN_OK
    assert lib().rdyn_rollout_adjoint(None, None, None, None, 0, 0, FAKE, 1 << 30) == RDYN_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", CHUNKED)
@pytest.mark.parametrize("integrator", [EULER, RK4])
def test_adjoint_workspace_of_the_chunked_route(name, integrator):
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 5000
    assert n > 10
    d = _desc(n, N, integrator=integrator)
    chunks = (1, 64, 1000, 16384, 100000)
    sizes = [_adj_query(chain, d, N, chunk) for chunk in chunks]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
    arrays = 18 if integrator == RK4 else 6   # the adjoint state, the product's seed and results; RK4: x_bar, the carry, three stage states
    for chunk, s in zip(chunks + (0,), sizes + [_adj_query(chain, d, N, 0)]):
        assert s >= _vjp_query(chain, chunk) + arrays * n * N * 8
    assert _adj_query(chain, d, 2 * N, 1000) > _adj_query(chain, d, N, 1000)
    assert _adj_query(chain, d, N, -5) == 0
    need = _adj_query(chain, d, 7, 1000)
    assert _adj(chain, 7, integrator=integrator, chunk_samples=1000, workspace_bytes=need - 1) == RDYN_ERR_INVALID_ARGUMENT
    assert _adj(chain, 7, integrator=integrator, chunk_samples=1000, workspace=None, workspace_bytes=need) == RDYN_ERR_INVALID_ARGUMENT
    assert _adj(chain, 7, integrator=integrator, workspace_bytes=0) == RDYN_ERR_INVALID_ARGUMENT
    assert _adj(chain, 0, integrator=integrator, workspace=None, workspace_bytes=0) == RDYN_OK


def test_python_bindings_exist():
    from rosdyn_amd import Chain, autograd
    assert callable(getattr(Chain, "getJointAccelerationVjp")) and callable(getattr(Chain, "rolloutAdjoint"))
    assert callable(autograd.joint_acceleration) and callable(autograd.rollout)
