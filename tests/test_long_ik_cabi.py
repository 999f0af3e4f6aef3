"""CPU tests (no GPU): argument checks of rdyn_local_ik_damped on chains with more than RDYN_MAX_SWEPT_JOINTS input joints
(rdyn_long_ik.hip).  Such chains have no reduced companion; they used to be refused with RDYN_ERR_UNSUPPORTED.  Nothing here
touches a device: every call either has no poses or fails its checks first."""
import ctypes as C

import pytest

from _cabi import FAKE, RDYN_ERR_INVALID_ARGUMENT, RDYN_OK
from rosdyn_amd.urdf_gen import generated_revolute_chain


def _call(chain, n_samples, T_target=FAKE, damping=1e-3, q=FAKE, max_iterations=10, toll=1e-6):
    from rosdyn_amd._lib import Batch, lib
    b = Batch()
    b.n_samples = n_samples
    b.q = q
    b.layout = 0
    b.device = 0
    w = (C.c_double * 6)(1, 1, 1, 1, 1, 1)
    return lib().rdyn_local_ik_damped(chain._h, C.byref(b), T_target, w, toll, damping, max_iterations, FAKE, FAKE, FAKE)


@pytest.mark.parametrize("nj", [11, 20, 32])
def test_long_ik_accepts_chains_with_more_than_ten_input_joints(nj):
    from rosdyn_amd import Chain
    chain = Chain(generated_revolute_chain(nj, 1000 + nj), "l0", "l%d" % nj)
    assert chain.getJointsNumber() == nj and chain.getActiveJointsNumber() == nj
    assert _call(chain, 0) == RDYN_OK
    assert _call(chain, 0, damping=0.0) == RDYN_OK       # undamped: served, every unconverged pose reports -1
    # poses without a target: an invalid argument, no longer an unsupported chain
    assert _call(chain, 5, T_target=None) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 5, q=None) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 0, damping=-1e-3) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 0, max_iterations=-1) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 0, toll=-1.0) == RDYN_ERR_INVALID_ARGUMENT


def test_long_ik_permuted_and_companion_routes_keep_their_checks():
    from rosdyn_amd import Chain
    chain = Chain(generated_revolute_chain(20, 1020), "l0", "l20")
    assert chain.setInputJointsName(["j%d" % i for i in (13, 0, 9, 4, 16, 1, 7, 19, 3, 10, 6, 12)])   # 12 inputs, any order
    assert _call(chain, 0) == RDYN_OK
    assert _call(chain, 3, T_target=None) == RDYN_ERR_INVALID_ARGUMENT
    assert chain.setInputJointsName(["j%d" % i for i in (5, 2, 11)])   # 3 inputs: the reduced companion serves it
    assert _call(chain, 0) == RDYN_OK
    assert _call(chain, 3, T_target=None) == RDYN_ERR_INVALID_ARGUMENT
    assert _call(chain, 0, damping=-1.0) == RDYN_ERR_INVALID_ARGUMENT
