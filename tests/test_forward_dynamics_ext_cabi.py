"""CPU tests (no GPU): argument checks and workspace queries of rdyn_forward_dynamics_ext and rdyn_rollout_ext (include/rdyn.h).
Nothing here touches a device: every call either has no samples or fails its checks first."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import FIXTURES, ROOT
from _cabi import CHUNKED, EULER, FAKE, RDYN_ERR_INVALID_ARGUMENT, RDYN_OK, RK4, SWEPT, _batch, _chain, _comps, _ext, _query, _rollout_desc as _desc
from _components import FRICTION1, SPRING


def _rollout(chain, N, ext, comps=None, n_comps=0, desc=True, chunk_samples=0, workspace=FAKE, workspace_bytes=None, q=FAKE, dq=FAKE, batch=True,
             layout=0, **kw):
    from rosdyn_amd._lib import lib
    b = _batch(N, q, dq, layout)
    d = _desc(chain.getActiveJointsNumber(), max(N, 0), **kw)
    px = C.byref(ext) if ext is not None else None
    if workspace_bytes is None:
        workspace_bytes = lib().rdyn_rollout_ext_workspace_bytes(chain._h, C.byref(d), px, max(N, 0), max(chunk_samples, 0))
    return lib().rdyn_rollout_ext(chain._h, C.byref(b) if batch else None, C.byref(d) if desc else None,
                                  C.cast(comps, C.c_void_p) if comps is not None else None, n_comps, px, chunk_samples, workspace, workspace_bytes)


def _fd(chain, N, ext, comps=None, n_comps=0, tau=FAKE, ddq=FAKE, status=FAKE, chunk_samples=0, workspace=FAKE, workspace_bytes=None, q=FAKE,
        dq=FAKE, batch=True, layout=0):
    from rosdyn_amd._lib import lib
    b = _batch(N, q, dq, layout)
    px = C.byref(ext) if ext is not None else None
    if workspace_bytes is None:
        workspace_bytes = lib().rdyn_forward_dynamics_ext_workspace_bytes(chain._h, px, max(chunk_samples, 0))
    return lib().rdyn_forward_dynamics_ext(chain._h, C.byref(b) if batch else None, C.cast(comps, C.c_void_p) if comps is not None else None,
                                           n_comps, px, tau, ddq, status, chunk_samples, workspace, workspace_bytes)


def test_the_symbols_exist_with_the_documented_signatures():
    from rosdyn_amd import _lib
    flat = re.sub(r"\s+", " ", open(ROOT + "/include/rdyn.h").read())
    assert ("int rdyn_forward_dynamics_ext(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_component* comps, int n_comps, "
            "const rdyn_ext_wrenches* ext, const double* tau, double* ddq, int32_t* status, int64_t chunk_samples, void* workspace, "
            "size_t workspace_bytes);") in flat
    assert ("int rdyn_rollout_ext(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_desc* desc, const rdyn_component* comps, "
            "int n_comps, const rdyn_ext_wrenches* ext, int64_t chunk_samples, void* workspace, size_t workspace_bytes);") in flat
    assert "size_t rdyn_forward_dynamics_ext_workspace_bytes(" in flat and "size_t rdyn_rollout_ext_workspace_bytes(" in flat
    l = _lib.lib()
    for name, nargs in (("rdyn_forward_dynamics_ext", 11), ("rdyn_rollout_ext", 9), ("rdyn_forward_dynamics_ext_workspace_bytes", 3),
                        ("rdyn_rollout_ext_workspace_bytes", 5)):
        assert getattr(l, name) is not None and len(_lib.SYMBOLS[name][1]) == nargs
    assert C.sizeof(_lib.ExtWrenches) == 24   # pointer, int32 + padding, int64
    # the two header comments that sent the caller away now point at the new calls
    assert "left for a follow-up" not in flat
    assert "rdyn_forward_dynamics_ext both" in flat and "rdyn_rollout_ext (below" in flat


@pytest.mark.parametrize("name", SWEPT + CHUNKED)
def test_no_samples_is_ok_and_every_refusal(name):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n, nj, N = chain.getActiveJointsNumber(), chain.getJointsNumber(), 7
    L = nj + 1
    arr = _comps([(FRICTION1, 0), (SPRING, n - 1)])
    # no samples; the tool is link nj, the base link 0
    for x in (None, _ext(None), _ext(), _ext(link=0), _ext(link=nj), _ext(step_stride=0)):
        for comps, k in ((None, 0), (arr, 2)):
            assert _rollout(chain, 0, x, comps, k) == RDYN_OK
            assert _rollout(chain, 0, x, comps, k, layout=1, integrator=EULER) == RDYN_OK
            assert _fd(chain, 0, x, comps, k) == RDYN_OK
            assert _fd(chain, 0, x, comps, k, q=None, dq=None, tau=None, ddq=None, status=None, workspace=None, workspace_bytes=0) == RDYN_OK
    # the link index
    for link in (-2, nj + 1, 1 << 20):
        for samples in (N, 0):
            assert _fd(chain, samples, _ext(link=link)) == RDYN_ERR_INVALID_ARGUMENT, link
            assert b"wrench link" in lib().rdyn_last_error()
            assert _rollout(chain, samples, _ext(link=link)) == RDYN_ERR_INVALID_ARGUMENT, link
            assert b"wrench link" in lib().rdyn_last_error()
    # the step stride: negative; not zero and smaller than one step's record (6 links N, or 6 N for one link)
    for x in (_ext(step_stride=-1), _ext(step_stride=6 * L * N - 1), _ext(step_stride=1), _ext(link=nj, step_stride=6 * N - 1),
              _ext(link=0, step_stride=-6 * N)):
        assert _rollout(chain, N, x) == RDYN_ERR_INVALID_ARGUMENT, (x.link, x.step_stride)
        assert b"step_stride" in lib().rdyn_last_error()
    assert _rollout(chain, 0, _ext(step_stride=-1)) == RDYN_ERR_INVALID_ARGUMENT
    # ... the smallest valid strides pass the wrench check: what is refused next is the component list
    bad = _comps([(FRICTION1, n)])
    for x in (_ext(step_stride=6 * L * N), _ext(link=nj, step_stride=6 * N), _ext(link=3 if nj >= 3 else 0, step_stride=0)):
        assert _rollout(chain, N, x, bad, 1) == RDYN_ERR_INVALID_ARGUMENT
        assert b"component" in lib().rdyn_last_error()
    # the forward-dynamics call does not read step_stride
    assert _fd(chain, N, _ext(step_stride=-1), bad, 1) == RDYN_ERR_INVALID_ARGUMENT and b"component" in lib().rdyn_last_error()
    # a bad link or stride without wrenches (w NULL) is not looked at: the call is the components call
    assert _fd(chain, 0, _ext(None, link=99)) == RDYN_OK and _rollout(chain, 0, _ext(None, link=99, step_stride=-5)) == RDYN_OK
    # every argument error of the base calls, with wrenches
    rollout_refusals = [
        {"desc": False}, {"tau": None}, {"q_end": None, "dq_end": None}, {"n_steps": -1},
        {"dt": 0.0}, {"dt": float("inf")}, {"dt": float("nan")}, {"integrator": 2}, {"integrator": -1},
        {"q_traj": FAKE, "traj_every": 0, "traj_step_stride": n * N}, {"q_traj": FAKE, "traj_every": 1, "traj_step_stride": n * N - 1},
        {"chunk_samples": -1}, {"q": None}, {"dq": None}, {"batch": False}, {"layout": 5},
        {"comps": None, "n_comps": 1}, {"comps": arr, "n_comps": -1}, {"comps": bad, "n_comps": 1}, {"comps": _comps([(7, 0)]), "n_comps": 1},
    ]
    fd_refusals = [{"tau": None}, {"ddq": None}, {"chunk_samples": -1}, {"q": None}, {"dq": None}, {"batch": False}, {"layout": 5},
                   {"comps": None, "n_comps": 31}, {"comps": bad, "n_comps": 1}]
    for x in (_ext(), _ext(link=nj), None):
        for kw in rollout_refusals:
            assert _rollout(chain, N, x, **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
            assert lib().rdyn_last_error()
        for kw in fd_refusals:
            assert _fd(chain, N, x, **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
            assert lib().rdyn_last_error()
        assert _rollout(chain, -1, x) == RDYN_ERR_INVALID_ARGUMENT and _fd(chain, -1, x) == RDYN_ERR_INVALID_ARGUMENT
    assert lib().rdyn_rollout_ext(None, None, None, None, 0, None, 0, FAKE, 1 << 30) == RDYN_ERR_INVALID_ARGUMENT
    assert lib().rdyn_forward_dynamics_ext(None, None, None, 0, None, FAKE, FAKE, FAKE, 0, FAKE, 1 << 30) == RDYN_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", SWEPT + CHUNKED)
def test_without_wrenches_the_workspace_queries_equal_the_base_queries(name):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    for x in (None, _ext(None, link=2, step_stride=77)):
        px = C.byref(x) if x is not None else None
        for chunk in (0, 1000, 20000):
            assert lib().rdyn_forward_dynamics_ext_workspace_bytes(chain._h, px, chunk) == lib().rdyn_forward_dynamics_workspace_bytes(chain._h, chunk)
            for integrator in (EULER, RK4):
                for N in (0, 7, 4096):
                    d = _desc(n, N, integrator=integrator)
                    assert lib().rdyn_rollout_ext_workspace_bytes(chain._h, C.byref(d), px, N, chunk) == _query(chain, d, N, chunk)
    # chains that stay on their route keep the base figure with wrenches too: the wrench recursion takes them, no buffer is added
    x = _ext()
    for chunk in (0, 1000):
        assert lib().rdyn_forward_dynamics_ext_workspace_bytes(chain._h, C.byref(x), chunk) == lib().rdyn_forward_dynamics_workspace_bytes(chain._h, chunk)
        d = _desc(n, 7)
        assert lib().rdyn_rollout_ext_workspace_bytes(chain._h, C.byref(d), C.byref(x), 7, chunk) == _query(chain, d, 7, chunk)


@pytest.mark.parametrize("name", CHUNKED)
def test_an_undersized_workspace_is_refused(name):
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    for x in (_ext(), _ext(link=1)):
        need = _query(chain, _desc(n, 7), 7, 1000)
        assert need > 0
        assert _rollout(chain, 7, x, chunk_samples=1000, workspace_bytes=need - 1) == RDYN_ERR_INVALID_ARGUMENT
        assert _rollout(chain, 7, x, chunk_samples=1000, workspace=None, workspace_bytes=need) == RDYN_ERR_INVALID_ARGUMENT
        assert _fd(chain, 7, x, chunk_samples=1000, workspace_bytes=1) == RDYN_ERR_INVALID_ARGUMENT
        assert _fd(chain, 7, x, chunk_samples=1000, workspace=None) == RDYN_ERR_INVALID_ARGUMENT


def test_a_long_chain_with_a_reduced_companion_takes_the_chunked_route_with_wrenches_only():
    """ur10_public_long: 6 input joints, more chain joints than the register kernels sweep.  Without wrenches it runs through its reduced
    companion (no workspace); with wrenches through the chunked route on the original chain: an image of n n + n doubles per sample."""
    from rosdyn_amd import Chain
    from rosdyn_amd._lib import lib
    chain = Chain(os.path.join(FIXTURES, "ur10_public_long.urdf"), "base_link", "tcp")
    n = chain.getActiveJointsNumber()
    assert chain.getJointsNumber() > 10 and n <= 10
    assert lib().rdyn_forward_dynamics_workspace_bytes(chain._h, 1000) == 0
    assert lib().rdyn_forward_dynamics_ext_workspace_bytes(chain._h, None, 1000) == 0
    x = _ext(link=chain.getJointsNumber())
    need = lib().rdyn_forward_dynamics_ext_workspace_bytes(chain._h, C.byref(x), 1000)
    assert need == (1000 * (n * n + n) * 8 + 255) // 256 * 256
    d = _desc(n, 7)
    assert _query(chain, d, 7, 1000) == 0
    assert lib().rdyn_rollout_ext_workspace_bytes(chain._h, C.byref(d), C.byref(x), 7, 1000) > need
    assert _fd(chain, 7, x, chunk_samples=1000, workspace_bytes=need - 1) == RDYN_ERR_INVALID_ARGUMENT
    assert _fd(chain, 0, x, chunk_samples=1000, workspace=None, workspace_bytes=0) == RDYN_OK


def test_python_keywords_exist():
    from rosdyn_amd import Chain
    for f in (Chain.rollout, Chain.getJointAcceleration):
        p = inspect.signature(f).parameters
        assert p["ext_wrenches"].default is None and p["ext_link"].default is None
