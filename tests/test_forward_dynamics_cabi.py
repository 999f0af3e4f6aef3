"""CPU tests (no GPU): argument checks and the workspace query of rdyn_forward_dynamics (ddq = M^-1 (tau - h), include/rdyn.h).
Nothing here touches a device: every call either has no samples or fails its checks first."""
import ctypes as C

import pytest

from _cabi import CHUNKED, FAKE, RDYN_ERR_INVALID_ARGUMENT, RDYN_OK, SWEPT, _chain


def _query(chain, chunk_samples=0):
    from rosdyn_amd._lib import lib
    return lib().rdyn_forward_dynamics_workspace_bytes(chain._h, chunk_samples)


def _call(chain, n_samples, q=FAKE, dq=FAKE, tau=FAKE, ddq=FAKE, status=FAKE, chunk_samples=0, workspace=FAKE, workspace_bytes=None,
          batch=True, layout=0):
    from rosdyn_amd._lib import Batch, lib
    b = Batch()
    b.n_samples = n_samples
    b.q = q
    b.dq = dq
    b.layout = layout
    b.device = 0
    if workspace_bytes is None:
        workspace_bytes = _query(chain, max(chunk_samples, 0))
    return lib().rdyn_forward_dynamics(chain._h, C.byref(b) if batch else None, tau, ddq, status, chunk_samples, workspace, workspace_bytes)


@pytest.mark.parametrize("name", SWEPT + CHUNKED)
def test_no_samples_is_ok_and_null_arguments_are_refused(name):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    assert _call(chain, 0) == RDYN_OK
    assert _call(chain, 0, q=None, dq=None, tau=None, ddq=None, status=None, workspace=None, workspace_bytes=0) == RDYN_OK
    assert _call(chain, 0, layout=1) == RDYN_OK
    for kw in ({"q": None}, {"dq": None}, {"tau": None}, {"ddq": None}, {"batch": False}):
        assert _call(chain, 7, **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
        assert lib().rdyn_last_error()
    assert _call(chain, -1) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 7, layout=5) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 0, chunk_samples=-1) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 7, chunk_samples=-64) == RDYN_ERR_INVALID_ARGUMENT
    assert lib().rdyn_forward_dynamics(None, None, FAKE, FAKE, FAKE, 0, FAKE, 1 << 30) == RDYN_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", SWEPT + ["rev10"])
def test_chains_swept_in_registers_need_no_workspace(name):
    chain = _chain(name)
    assert chain.getActiveJointsNumber() <= 10
    for chunk in (0, 1, 16384, 1 << 20):
        assert _query(chain, chunk) == 0


@pytest.mark.parametrize("name", CHUNKED)
def test_workspace_of_the_chunked_route(name):
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    assert n > 10
    sizes = [_query(chain, chunk) for chunk in (1, 64, 1000, 16384, 100000)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
    for chunk, s in zip((1, 64, 1000, 16384, 100000), sizes):
        assert s >= chunk * (n * n + n) * 8
    # the default chunk: an image within 128 MiB, at least 16 384 samples
    assert _query(chain, 0) >= 16384 * (n * n + n) * 8
    assert _query(chain, 0) <= max(128 << 20, 16384 * (n * n + n) * 8) + 256
    assert _query(chain, -5) == 0
    # an undersized or missing workspace is refused before any device work
    need = _query(chain, 1000)
    assert _call(chain, 7, chunk_samples=1000, workspace_bytes=need - 1) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 7, chunk_samples=1000, workspace=None, workspace_bytes=need) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 7, workspace_bytes=0) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 0, workspace=None, workspace_bytes=0) == RDYN_OK


def test_python_binding_exists():
    from rosdyn_amd import Chain
    assert callable(getattr(Chain, "getJointAcceleration"))
