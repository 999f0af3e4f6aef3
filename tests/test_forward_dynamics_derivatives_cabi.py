"""CPU tests (no GPU): argument checks and the workspace query of rdyn_forward_dynamics_derivatives (dDDq/dq, dDDq/dDq, M^-1;
include/rdyn.h).  Nothing here touches a device: every call either has no samples or fails its checks first."""
import ctypes as C

import pytest

from _cabi import CHUNKED, FAKE, RDYN_ERR_INVALID_ARGUMENT, RDYN_OK, SWEPT, _chain, _comps
from _components import FRICTION1, FRICTION2, SPRING

ONE_SWEPT, ONE_CHUNKED = SWEPT[0], CHUNKED[1]


def _query(chain, chunk_samples=0):
    from rosdyn_amd._lib import lib
    return lib().rdyn_forward_dynamics_derivatives_workspace_bytes(chain._h, chunk_samples)


def _call(chain, n_samples, comps=None, n_comps=0, q=FAKE, dq=FAKE, tau=FAKE, ddq=FAKE, dddq_dq=FAKE, dddq_dv=FAKE, minv=FAKE, status=FAKE,
          chunk_samples=0, workspace=FAKE, workspace_bytes=None, batch=True, layout=0):
    from rosdyn_amd._lib import Batch, lib
    b = Batch()
    b.n_samples, b.q, b.dq, b.layout, b.device = n_samples, q, dq, layout, 0
    if workspace_bytes is None:
        workspace_bytes = _query(chain, max(chunk_samples, 0))
    return lib().rdyn_forward_dynamics_derivatives(chain._h, C.byref(b) if batch else None, C.cast(comps, C.c_void_p) if comps is not None else None,
                                                   n_comps, tau, ddq, dddq_dq, dddq_dv, minv, status, chunk_samples, workspace, workspace_bytes)


def test_the_symbols_and_the_python_method_exist():
    from rosdyn_amd import Chain, _lib
    for name, nargs in (("rdyn_forward_dynamics_derivatives_workspace_bytes", 2), ("rdyn_forward_dynamics_derivatives", 13)):
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs
        assert getattr(_lib.lib(), name) is not None
    assert callable(getattr(Chain, "getJointAccelerationDerivatives"))


@pytest.mark.parametrize("name", [ONE_SWEPT, ONE_CHUNKED])
def test_no_samples_is_ok_with_any_pointers(name):
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    arr = _comps([(FRICTION1, 0), (SPRING, 0), (FRICTION2, n - 1)])
    for comps, k in ((None, 0), (arr, 3), (arr, 0)):
        assert _call(chain, 0, comps, k) == RDYN_OK
        assert _call(chain, 0, comps, k, layout=1) == RDYN_OK
        assert _call(chain, 0, comps, k, q=None, dq=None, tau=None, ddq=None, dddq_dq=None, dddq_dv=None, minv=None, status=None,
                     workspace=None, workspace_bytes=0) == RDYN_OK


@pytest.mark.parametrize("name", [ONE_SWEPT, ONE_CHUNKED])
def test_every_refusal_is_an_invalid_argument_with_a_message(name):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 7
    good = [(FRICTION1, 0), (SPRING, 0), (FRICTION2, n - 1)]
    arr = _comps(good)
    # the component list: the rules of rdyn_forward_dynamics_components, with and without samples
    bad_lists = [
        (_comps([(3, 0)]), 1), (_comps([(-1, 0)]), 1),
        (_comps([(FRICTION1, n)]), 1), (_comps([(SPRING, -1)]), 1),
        (_comps(good + [(FRICTION2, n)]), 4),
        (_comps([(FRICTION1, 0)] * 31), 31),
        (None, 1), (None, 30),
        (arr, -1),
    ]
    for comps, k in bad_lists:
        for samples in (N, 0):
            assert _call(chain, samples, comps, k) == RDYN_ERR_INVALID_ARGUMENT, (k, samples)
            assert lib().rdyn_last_error()
    assert _call(chain, 0, _comps([(FRICTION1, 0)] * 30), 30) == RDYN_OK   # 30 are allowed
    refusals = [{"tau": None}, {"ddq": None}, {"dddq_dq": None, "dddq_dv": None, "minv": None}, {"chunk_samples": -1}, {"q": None},
                {"dq": None}, {"batch": False}, {"layout": 5}]
    for comps, k in ((arr, len(good)), (None, 0)):
        for kw in refusals:
            assert _call(chain, N, comps, k, **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
            assert lib().rdyn_last_error()
        assert _call(chain, -1, comps, k) == RDYN_ERR_INVALID_ARGUMENT
        assert _call(chain, 0, comps, k, chunk_samples=-1) == RDYN_ERR_INVALID_ARGUMENT
    assert lib().rdyn_forward_dynamics_derivatives(None, None, None, 0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0, FAKE, 1 << 30) == RDYN_ERR_INVALID_ARGUMENT
    assert lib().rdyn_last_error()


@pytest.mark.parametrize("name", SWEPT + ["rev10"])
def test_chains_swept_in_registers_need_no_workspace(name):
    chain = _chain(name)
    for chunk in (0, 1, 16384, 1 << 20):
        assert _query(chain, chunk) == 0
    assert _call(chain, 0, workspace=None, workspace_bytes=0) == RDYN_OK


@pytest.mark.parametrize("name", CHUNKED)
def test_workspace_of_the_chunked_route(name):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    for chunk in (0, 1, 64, 1000, 16384, 100000):
        assert _query(chain, chunk) >= lib().rdyn_forward_dynamics_workspace_bytes(chain._h, chunk) > 0
    assert _query(chain, -5) == 0
    # an undersized or missing workspace is refused against this call's own query, before any device work
    need = _query(chain, 1000)
    assert _call(chain, 7, chunk_samples=1000, workspace_bytes=need - 1) == RDYN_ERR_INVALID_ARGUMENT
    assert lib().rdyn_last_error()
    assert _call(chain, 7, chunk_samples=1000, workspace=None, workspace_bytes=need) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 7, workspace_bytes=0) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 0, workspace=None, workspace_bytes=0) == RDYN_OK


def test_the_python_wrapper_refuses_a_bad_want():
    chain = _chain(ONE_SWEPT)
    for want in ((), ("dq", "dq"), ("M",), ("dq", "tau"), "x", ["dv", "dtau", "dv"]):
        with pytest.raises(ValueError):
            chain.getJointAccelerationDerivatives(None, None, None, want=want)
