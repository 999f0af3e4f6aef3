"""CPU tests (no GPU): argument checks of rdyn_joint_torque_derivatives (dtau/dq, dtau/dDq, M = dtau/dDDq; include/rdyn.h).
Nothing here touches a device: every call either has no samples or fails its checks first."""
import ctypes as C

import pytest

from _cabi import CHUNKED, FAKE, RDYN_ERR_INVALID_ARGUMENT, RDYN_OK, SWEPT, _chain


def _call(chain, n_samples, q=FAKE, dq=FAKE, ddq=FAKE, dtau_dq=FAKE, dtau_dv=FAKE, M=FAKE, batch=True, layout=0):
    from rosdyn_amd._lib import Batch, lib
    b = Batch()
    b.n_samples = n_samples
    b.q = q
    b.dq = dq
    b.ddq = ddq
    b.layout = layout
    b.device = 0
    return lib().rdyn_joint_torque_derivatives(chain._h, C.byref(b) if batch else None, dtau_dq, dtau_dv, M)


def test_symbol_and_python_binding_exist():
    from rosdyn_amd import Chain
    from rosdyn_amd._lib import SYMBOLS, lib
    assert "rdyn_joint_torque_derivatives" in SYMBOLS
    assert getattr(lib(), "rdyn_joint_torque_derivatives")
    assert callable(getattr(Chain, "getJointTorqueDerivatives"))


@pytest.mark.parametrize("name", SWEPT + CHUNKED)
def test_no_samples_is_ok_and_bad_arguments_are_refused(name):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    for layout in (0, 1):
        assert _call(chain, 0, layout=layout) == RDYN_OK
        assert _call(chain, 0, q=None, dq=None, ddq=None, dtau_dq=None, dtau_dv=None, M=None, layout=layout) == RDYN_OK
    refusals = ({"q": None}, {"dq": None}, {"ddq": None}, {"batch": False}, {"dtau_dq": None, "dtau_dv": None, "M": None},
                {"layout": 5}, {"layout": -1})
    for kw in refusals:
        assert _call(chain, 7, **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
        assert lib().rdyn_last_error(), kw
    assert _call(chain, -1) == RDYN_ERR_INVALID_ARGUMENT
    assert lib().rdyn_last_error()
    assert _call(chain, -1, dtau_dq=None, dtau_dv=None, M=None) == RDYN_ERR_INVALID_ARGUMENT
    assert lib().rdyn_joint_torque_derivatives(None, None, FAKE, FAKE, FAKE) == RDYN_ERR_INVALID_ARGUMENT
    assert lib().rdyn_last_error()


@pytest.mark.parametrize("name", ["ur10_like", "rev20"])
def test_python_wrapper_refuses_a_bad_selection(name):
    chain = _chain(name)
    for want in ((), ("dq", "dq"), ("x",), "tau"):
        with pytest.raises(ValueError):
            chain.getJointTorqueDerivatives(None, None, None, want=want)
