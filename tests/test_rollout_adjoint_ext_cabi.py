"""CPU tests (no GPU): argument checks, routing and workspace queries of rdyn_forward_dynamics_vjp_ext and rdyn_rollout_adjoint_ext
(include/rdyn.h).  Nothing here touches a device: every call either has no samples or fails its checks first."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import FIXTURES, ROOT
from _cabi import (CHUNKED, EULER, FAKE, RDYN_ERR_INVALID_ARGUMENT, RDYN_ERR_UNSUPPORTED, RDYN_OK, RK4,
                   SWEPT, _adj_query, _adjoint_desc as _desc, _batch, _chain, _comp, _ext, _vjp_query)


def _gext(gw=FAKE, step_stride=0):
    from rosdyn_amd._lib import ExtWrenchGradient
    g = ExtWrenchGradient()
    g.gw, g.step_stride = gw, step_stride
    return g


def _vjp(chain, N, ext, q=FAKE, dq=FAKE, tau=FAKE, seed=FAKE, q_bar=FAKE, dq_bar=FAKE, tau_bar=FAKE, ext_bar=FAKE, ddq=FAKE, status=FAKE,
         comps=None, n_comps=0, chunk_samples=0, workspace=FAKE, workspace_bytes=None, batch=True, layout=0):
    from rosdyn_amd._lib import lib
    b = _batch(N, q, dq, layout)
    px = C.byref(ext) if ext is not None else None
    if workspace_bytes is None:
        workspace_bytes = lib().rdyn_forward_dynamics_vjp_ext_workspace_bytes(chain._h, px, max(chunk_samples, 0))
    return lib().rdyn_forward_dynamics_vjp_ext(chain._h, C.byref(b) if batch else None, comps, n_comps, px, tau, seed, q_bar, dq_bar, tau_bar,
                                               ext_bar, ddq, status, chunk_samples, workspace, workspace_bytes)


def _adj(chain, N, ext, gext=None, desc=True, comps=None, n_comps=0, chunk_samples=0, workspace=FAKE, workspace_bytes=None, q=FAKE, dq=FAKE,
         batch=True, layout=0, **kw):
    from rosdyn_amd._lib import lib
    b = _batch(N, q, dq, layout)
    d = _desc(chain.getActiveJointsNumber(), max(N, 0), **kw)
    px = C.byref(ext) if ext is not None else None
    pg = C.byref(gext) if gext is not None else None
    if workspace_bytes is None:
        workspace_bytes = lib().rdyn_rollout_adjoint_ext_workspace_bytes(chain._h, C.byref(d), px, max(N, 0), max(chunk_samples, 0))
    return lib().rdyn_rollout_adjoint_ext(chain._h, C.byref(b) if batch else None, C.byref(d) if desc else None, comps, n_comps, px, pg,
                                          chunk_samples, workspace, workspace_bytes)


def _err():
    from rosdyn_amd._lib import lib
    return lib().rdyn_last_error()


def test_the_symbols_exist_with_the_documented_signatures():
    from rosdyn_amd import _lib
    flat = re.sub(r"\s+", " ", open(ROOT + "/include/rdyn.h").read())
    assert ("int rdyn_forward_dynamics_vjp_ext(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_component* comps, int n_comps, "
            "const rdyn_ext_wrenches* ext, const double* tau, const double* ddq_bar, double* q_bar, double* dq_bar, double* tau_bar, "
            "double* ext_bar, double* ddq, int32_t* status, int64_t chunk_samples, void* workspace, size_t workspace_bytes);") in flat
    assert ("int rdyn_rollout_adjoint_ext(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_adjoint_desc* desc, "
            "const rdyn_component* comps, int n_comps, const rdyn_ext_wrenches* ext, const rdyn_ext_wrench_gradient* gext, "
            "int64_t chunk_samples, void* workspace, size_t workspace_bytes);") in flat
    assert "size_t rdyn_forward_dynamics_vjp_ext_workspace_bytes(" in flat and "size_t rdyn_rollout_adjoint_ext_workspace_bytes(" in flat
    # both calls stand behind rdyn_rollout_adjoint_parameters, and the header names the follow-up
    assert flat.index("int rdyn_rollout_adjoint_parameters(") < flat.index("size_t rdyn_forward_dynamics_vjp_ext_workspace_bytes(")
    assert "mode with wrenches is the follow-up" in flat
    l = _lib.lib()
    for name, nargs in (("rdyn_forward_dynamics_vjp_ext", 16), ("rdyn_rollout_adjoint_ext", 10),
                        ("rdyn_forward_dynamics_vjp_ext_workspace_bytes", 3), ("rdyn_rollout_adjoint_ext_workspace_bytes", 5)):
        assert getattr(l, name) is not None and len(_lib.SYMBOLS[name][1]) == nargs
    assert C.sizeof(_lib.ExtWrenchGradient) == 16


@pytest.mark.parametrize("name", SWEPT + ["rev10"])
def test_with_wrenches_every_refusal_of_a_swept_chain(name):
    chain = _chain(name)
    n, nj, N = chain.getActiveJointsNumber(), chain.getJointsNumber(), 7
    L = nj + 1
    one = _comp()
    bad_joint = _comp(joint=n)
    # no samples; the tool is link nj, the base link 0
    for x in (_ext(), _ext(link=0), _ext(link=nj)):
        for g in (None, _gext(None), _gext(), _gext(step_stride=6 * L * N)):
            assert _adj(chain, 0, x, g) == RDYN_OK
            assert _adj(chain, 0, x, g, layout=1, integrator=EULER) == RDYN_OK
        assert _vjp(chain, 0, x) == RDYN_OK
        assert _vjp(chain, 0, x, q=None, dq=None, tau=None, seed=None, q_bar=None, dq_bar=None, tau_bar=None, ext_bar=None, ddq=None, status=None,
                    workspace=None, workspace_bytes=0) == RDYN_OK
    # the link range
    for link in (-2, nj + 1, 1 << 20):
        for samples in (N, 0):
            assert _vjp(chain, samples, _ext(link=link)) == RDYN_ERR_INVALID_ARGUMENT and b"wrench link" in _err()
            assert _adj(chain, samples, _ext(link=link)) == RDYN_ERR_INVALID_ARGUMENT and b"wrench link" in _err()
    # the wrench step stride (the adjoint alone reads it)
    for x in (_ext(step_stride=-1), _ext(step_stride=6 * L * N - 1), _ext(step_stride=1), _ext(link=nj, step_stride=6 * N - 1)):
        assert _adj(chain, N, x) == RDYN_ERR_INVALID_ARGUMENT and b"wrench step_stride" in _err()
        assert _vjp(chain, N, x, comps=C.addressof(bad_joint), n_comps=1) == RDYN_ERR_INVALID_ARGUMENT and b"component" in _err()
    # the gradient's step stride: negative, or not zero and below one step's record
    for x, g in ((_ext(), _gext(step_stride=-1)), (_ext(), _gext(step_stride=6 * L * N - 1)), (_ext(), _gext(step_stride=1)),
                 (_ext(link=nj), _gext(step_stride=6 * N - 1)), (_ext(link=0), _gext(step_stride=-6 * N))):
        assert _adj(chain, N, x, g) == RDYN_ERR_INVALID_ARGUMENT and b"wrench-gradient step_stride" in _err()
    # ... the smallest valid strides pass: what is refused next is the component list; without gw the stride is not read
    for x, g in ((_ext(step_stride=6 * L * N), _gext(step_stride=6 * L * N)), (_ext(link=nj, step_stride=6 * N), _gext(step_stride=6 * N)),
                 (_ext(), _gext(step_stride=0)), (_ext(), _gext(None, step_stride=-3))):
        assert _adj(chain, N, x, g, comps=C.addressof(bad_joint), n_comps=1) == RDYN_ERR_INVALID_ARGUMENT and b"component" in _err()
    # every product / every output null with samples; one of them is enough
    assert _vjp(chain, N, _ext(), q_bar=None, dq_bar=None, tau_bar=None, ext_bar=None) == RDYN_ERR_INVALID_ARGUMENT and b"every product" in _err()
    assert _vjp(chain, N, _ext(), q_bar=None, dq_bar=None, tau_bar=None, comps=C.addressof(bad_joint), n_comps=1) == RDYN_ERR_INVALID_ARGUMENT
    assert b"component" in _err()
    assert _adj(chain, N, _ext(), _gext(None), gq0=None, gdq0=None, gtau=None) == RDYN_ERR_INVALID_ARGUMENT and b"every output" in _err()
    assert _adj(chain, N, _ext(), None, gq0=None, gdq0=None, gtau=None) == RDYN_ERR_INVALID_ARGUMENT and b"every output" in _err()
    assert _adj(chain, N, _ext(), _gext(), gq0=None, gdq0=None, gtau=None, comps=C.addressof(bad_joint), n_comps=1) == RDYN_ERR_INVALID_ARGUMENT
    assert b"component" in _err()
    # every argument error of the base calls, with wrenches
    for x in (_ext(), _ext(link=nj)):
        for kw in ({"q": None}, {"dq": None}, {"batch": False}, {"tau": None}, {"seed": None}, {"chunk_samples": -1}, {"layout": 5},
                   {"comps": None, "n_comps": 1}, {"comps": C.addressof(one), "n_comps": -1}, {"comps": C.addressof(one), "n_comps": 31}):
            assert _vjp(chain, N, x, **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
            assert _err()
        for kw in ({"desc": False}, {"n_steps": -1}, {"dt": 0.0}, {"dt": float("nan")}, {"integrator": 2}, {"tau": None}, {"q_traj": None},
                   {"traj_step_stride": n * N - 1}, {"gtraj_step_stride": n * N - 1}, {"gtau_step_stride": 1}, {"chunk_samples": -1},
                   {"q": None}, {"dq": None}, {"batch": False}, {"layout": 5}, {"comps": None, "n_comps": 1}):
            assert _adj(chain, N, x, _gext(), **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
            assert _err()
        assert _vjp(chain, -1, x) == RDYN_ERR_INVALID_ARGUMENT and _adj(chain, -1, x) == RDYN_ERR_INVALID_ARGUMENT
    # one launch, no workspace: the queries are 0 and a null workspace is accepted
    x = _ext()
    from rosdyn_amd._lib import lib
    for chunk in (0, 1000):
        assert lib().rdyn_forward_dynamics_vjp_ext_workspace_bytes(chain._h, C.byref(x), chunk) == 0
        for integrator in (EULER, RK4):
            d = _desc(n, N, integrator=integrator)
            assert lib().rdyn_rollout_adjoint_ext_workspace_bytes(chain._h, C.byref(d), C.byref(x), N, chunk) == 0


@pytest.mark.parametrize("name", SWEPT + CHUNKED)
def test_without_wrenches_the_calls_and_the_queries_are_the_base_ones(name):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 7
    for x in (None, _ext(None, link=99, step_stride=-5)):
        px = C.byref(x) if x is not None else None
        for chunk in (0, 1000, 20000):
            assert lib().rdyn_forward_dynamics_vjp_ext_workspace_bytes(chain._h, px, chunk) == _vjp_query(chain, chunk)
            for integrator in (EULER, RK4):
                for samples in (0, 7, 4096):
                    d = _desc(n, samples, integrator=integrator)
                    assert lib().rdyn_rollout_adjoint_ext_workspace_bytes(chain._h, C.byref(d), px, samples, chunk) == _adj_query(chain, d, samples,
                                                                                                                                chunk)
        # a bad link or stride without w is not looked at; the base calls' refusals are the base calls'
        assert _vjp(chain, 0, x, ext_bar=None) == RDYN_OK and _adj(chain, 0, x) == RDYN_OK and _adj(chain, 0, x, _gext(None, -7)) == RDYN_OK
        assert _vjp(chain, N, x, ext_bar=None, tau=None) == RDYN_ERR_INVALID_ARGUMENT and b"rdyn_forward_dynamics_vjp:" in _err()
        assert _adj(chain, N, x, dt=0.0) == RDYN_ERR_INVALID_ARGUMENT and b"rdyn_rollout_adjoint:" in _err()
        # a gradient with respect to wrenches that are not there
        for samples in (0, N):
            assert _vjp(chain, samples, x) == RDYN_ERR_INVALID_ARGUMENT and b"ext_bar without external wrenches" in _err()
            assert _adj(chain, samples, x, _gext()) == RDYN_ERR_INVALID_ARGUMENT and b"wrench gradient without external wrenches" in _err()


def _long():
    from rosdyn_amd import Chain
    chain = Chain(os.path.join(FIXTURES, "ur10_public_long.urdf"), "base_link", "tcp")
    assert chain.getJointsNumber() > 10 and chain.getActiveJointsNumber() <= 10
    return chain


@pytest.mark.parametrize("name", CHUNKED + ["ur10_public_long"])
def test_with_wrenches_the_chunked_chains_are_unsupported_and_the_message_says_so(name):
    chain = _long() if name == "ur10_public_long" else _chain(name)
    nj, N = chain.getJointsNumber(), 7
    for x in (_ext(), _ext(link=nj), _ext(link=0)):
        for samples in (N, 0):
            assert _vjp(chain, samples, x) == RDYN_ERR_UNSUPPORTED
            assert b"rdyn_forward_dynamics_vjp_ext" in _err() and b"chunked route" in _err() and b"not served yet" in _err()
            assert _adj(chain, samples, x, _gext()) == RDYN_ERR_UNSUPPORTED
            assert b"rdyn_rollout_adjoint_ext" in _err() and b"chunked route" in _err() and b"without wrenches the call serves them" in _err()
    # the argument errors still come first
    assert _vjp(chain, N, _ext(link=nj + 1)) == RDYN_ERR_INVALID_ARGUMENT and _adj(chain, N, _ext(step_stride=-1)) == RDYN_ERR_INVALID_ARGUMENT
    assert _vjp(chain, N, _ext(), tau=None) == RDYN_ERR_INVALID_ARGUMENT and _adj(chain, N, _ext(), dt=0.0) == RDYN_ERR_INVALID_ARGUMENT
    # without wrenches these chains are served as before
    assert _vjp(chain, 0, None, ext_bar=None) == RDYN_OK and _adj(chain, 0, None) == RDYN_OK


def test_python_keywords_exist():
    from rosdyn_amd import Chain, autograd
    p = inspect.signature(Chain.getJointAccelerationVjp).parameters
    assert p["ext_wrenches"].default is None and p["ext_link"].default is None
    p = inspect.signature(Chain.rolloutAdjoint).parameters
    assert p["ext_wrenches"].default is None and p["ext_link"].default is None and p["want_ext"].default is False and p["sum_ext"].default is False
    for f in (autograd.joint_acceleration, autograd.rollout):
        p = inspect.signature(f).parameters
        assert p["ext_wrenches"].default is None and p["ext_link"].default is None
    assert issubclass(autograd.JointAccelerationExtFunction, __import__("torch").autograd.Function)
    assert issubclass(autograd.RolloutExtFunction, __import__("torch").autograd.Function)
