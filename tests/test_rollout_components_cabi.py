"""CPU tests (no GPU): argument checks of rdyn_forward_dynamics_components and rdyn_rollout_components (include/rdyn.h).
Nothing here touches a device: every call either has no samples or fails its checks first."""
import ctypes as C
import inspect
import re

import pytest

from conftest import ROOT
from _cabi import CHUNKED, EULER, FAKE, RDYN_ERR_INVALID_ARGUMENT, RDYN_OK, RK4, SWEPT, _chain, _comps, _query, _rollout_desc as _desc
from _components import FRICTION1, FRICTION2, SPRING


def _rollout(chain, N, comps, n_comps, desc=True, chunk_samples=0, workspace=FAKE, workspace_bytes=None, q=FAKE, dq=FAKE, batch=True, layout=0, **kw):
    from rosdyn_amd._lib import Batch, lib
    b = Batch()
    b.n_samples, b.q, b.dq, b.layout, b.device = N, q, dq, layout, 0
    d = _desc(chain.getActiveJointsNumber(), max(N, 0), **kw)
    if workspace_bytes is None:
        workspace_bytes = _query(chain, d, max(N, 0), max(chunk_samples, 0))
    return lib().rdyn_rollout_components(chain._h, C.byref(b) if batch else None, C.byref(d) if desc else None,
                                         C.cast(comps, C.c_void_p) if comps is not None else None, n_comps, chunk_samples, workspace, workspace_bytes)


def _fd(chain, N, comps, n_comps, tau=FAKE, ddq=FAKE, status=FAKE, chunk_samples=0, workspace=FAKE, workspace_bytes=None, q=FAKE, dq=FAKE,
        batch=True, layout=0):
    from rosdyn_amd._lib import Batch, lib
    b = Batch()
    b.n_samples, b.q, b.dq, b.layout, b.device = N, q, dq, layout, 0
    if workspace_bytes is None:
        workspace_bytes = lib().rdyn_forward_dynamics_workspace_bytes(chain._h, max(chunk_samples, 0))
    return lib().rdyn_forward_dynamics_components(chain._h, C.byref(b) if batch else None, C.cast(comps, C.c_void_p) if comps is not None else None,
                                                  n_comps, tau, ddq, status, chunk_samples, workspace, workspace_bytes)


def test_the_symbols_exist_with_the_documented_signatures():
    from rosdyn_amd import _lib
    hdr = open(ROOT + "/include/rdyn.h").read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int rdyn_forward_dynamics_components(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_component* comps, int n_comps, "
            "const double* tau, double* ddq, int32_t* status, int64_t chunk_samples, void* workspace, size_t workspace_bytes);") in flat
    assert ("int rdyn_rollout_components(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_desc* desc, "
            "const rdyn_component* comps, int n_comps, int64_t chunk_samples, void* workspace, size_t workspace_bytes);") in flat
    # the base calls and the descriptor are what they were
    assert ("int rdyn_rollout(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_desc* desc, int64_t chunk_samples, "
            "void* workspace, size_t workspace_bytes);") in flat
    assert ("int rdyn_forward_dynamics(const rdyn_chain* chain, const rdyn_batch* batch, const double* tau, double* ddq, int32_t* status, "
            "int64_t chunk_samples, void* workspace, size_t workspace_bytes);") in flat
    l = _lib.lib()
    for name, nargs in (("rdyn_forward_dynamics_components", 10), ("rdyn_rollout_components", 8)):
        assert getattr(l, name) is not None and len(_lib.SYMBOLS[name][1]) == nargs
    assert C.sizeof(_lib.RolloutDesc) == 88


@pytest.mark.parametrize("name", SWEPT + CHUNKED)
def test_no_samples_is_ok_and_every_refusal(name):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 7
    good = [(FRICTION1, 0), (SPRING, 0), (FRICTION2, n - 1)]
    arr = _comps(good)
    for comps, k in ((arr, len(good)), (None, 0), (arr, 0)):
        assert _rollout(chain, 0, comps, k) == RDYN_OK
        assert _rollout(chain, 0, comps, k, layout=1, integrator=EULER) == RDYN_OK
        assert _rollout(chain, 0, comps, k, q=None, dq=None, q_end=None, dq_end=None, status=None, workspace=None, workspace_bytes=0) == RDYN_OK
        assert _fd(chain, 0, comps, k) == RDYN_OK
        assert _fd(chain, 0, comps, k, q=None, dq=None, tau=None, ddq=None, status=None, workspace=None, workspace_bytes=0) == RDYN_OK
    bad_lists = [
        (_comps([(3, 0)]), 1), (_comps([(-1, 0)]), 1),                                # a bad component type
        (_comps([(FRICTION1, n)]), 1), (_comps([(SPRING, -1)]), 1),                   # joint out of range
        (_comps(good + [(FRICTION2, n)]), 4),                                         # ... in the last entry
        (_comps([(FRICTION1, 0)] * 31), 31),                                          # more than 30 components
        (None, 1), (None, 30),                                                        # NULL comps with n_comps > 0
        (arr, -1),
    ]
    for comps, k in bad_lists:
        for samples in (N, 0):
            assert _rollout(chain, samples, comps, k) == RDYN_ERR_INVALID_ARGUMENT, (k, samples)
            assert lib().rdyn_last_error()
            assert _fd(chain, samples, comps, k) == RDYN_ERR_INVALID_ARGUMENT, (k, samples)
            assert lib().rdyn_last_error()
    assert _rollout(chain, 0, _comps([(FRICTION1, 0)] * 30), 30) == RDYN_OK   # 30 are allowed
    # each error of the base calls, with and without components
    rollout_refusals = [
        {"desc": False}, {"tau": None}, {"q_end": None, "dq_end": None}, {"n_steps": -1},
        {"dt": 0.0}, {"dt": float("inf")}, {"dt": float("-inf")}, {"dt": float("nan")},
        {"integrator": 2}, {"integrator": -1},
        {"q_traj": FAKE, "traj_every": 0, "traj_step_stride": n * N},
        {"dq_traj": FAKE, "traj_every": -3, "traj_step_stride": n * N},
        {"q_traj": FAKE, "traj_every": 1, "traj_step_stride": n * N - 1},
        {"dq_traj": FAKE, "traj_every": 2, "traj_step_stride": 0},
        {"chunk_samples": -1}, {"q": None}, {"dq": None}, {"batch": False}, {"layout": 5},
    ]
    fd_refusals = [{"tau": None}, {"ddq": None}, {"chunk_samples": -1}, {"q": None}, {"dq": None}, {"batch": False}, {"layout": 5}]
    for comps, k in ((arr, len(good)), (None, 0)):
        for kw in rollout_refusals:
            assert _rollout(chain, N, comps, k, **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
            assert lib().rdyn_last_error()
        for kw in fd_refusals:
            assert _fd(chain, N, comps, k, **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
            assert lib().rdyn_last_error()
        assert _rollout(chain, -1, comps, k) == RDYN_ERR_INVALID_ARGUMENT and _fd(chain, -1, comps, k) == RDYN_ERR_INVALID_ARGUMENT
    assert lib().rdyn_rollout_components(None, None, None, None, 0, 0, FAKE, 1 << 30) == RDYN_ERR_INVALID_ARGUMENT
    assert lib().rdyn_forward_dynamics_components(None, None, None, 0, FAKE, FAKE, FAKE, 0, FAKE, 1 << 30) == RDYN_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", CHUNKED)
def test_the_workspace_queries_answer_for_the_new_calls(name):
    """an undersized or missing workspace is refused by the base calls' own figure; nothing more is asked for with components"""
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    arr = _comps([(FRICTION1, 0), (SPRING, n - 1)])
    for integrator in (EULER, RK4):
        need = _query(chain, _desc(n, 7, integrator=integrator), 7, 1000)
        assert need > 0
        assert _rollout(chain, 7, arr, 2, integrator=integrator, chunk_samples=1000, workspace_bytes=need - 1) == RDYN_ERR_INVALID_ARGUMENT
        assert _rollout(chain, 7, arr, 2, integrator=integrator, chunk_samples=1000, workspace=None, workspace_bytes=need) == RDYN_ERR_INVALID_ARGUMENT
        # with exactly the queried size the only thing left to refuse is the list
        assert _rollout(chain, 7, _comps([(FRICTION1, n)]), 1, integrator=integrator, chunk_samples=1000, workspace_bytes=need) == RDYN_ERR_INVALID_ARGUMENT
        assert b"component" in lib().rdyn_last_error()
    need = lib().rdyn_forward_dynamics_workspace_bytes(chain._h, 1000)
    assert need > 0
    assert _fd(chain, 7, arr, 2, chunk_samples=1000, workspace_bytes=need - 1) == RDYN_ERR_INVALID_ARGUMENT
    assert _fd(chain, 7, arr, 2, chunk_samples=1000, workspace=None, workspace_bytes=need) == RDYN_ERR_INVALID_ARGUMENT
    assert _fd(chain, 7, _comps([(5, 0)]), 1, chunk_samples=1000, workspace_bytes=need) == RDYN_ERR_INVALID_ARGUMENT
    assert b"component" in lib().rdyn_last_error()


@pytest.mark.parametrize("name", SWEPT + ["rev10"])
def test_register_route_needs_no_workspace(name):
    chain = _chain(name)
    arr = _comps([(FRICTION1, 0)])
    assert _rollout(chain, 0, arr, 1, workspace=None, workspace_bytes=0) == RDYN_OK
    assert _query(chain, _desc(chain.getActiveJointsNumber(), 4096), 4096, 0) == 0


def test_python_keywords_exist():
    from rosdyn_amd import Chain
    assert "components" in inspect.signature(Chain.rollout).parameters
    assert "components" in inspect.signature(Chain.getJointAcceleration).parameters
    assert inspect.signature(Chain.rollout).parameters["components"].default is None
