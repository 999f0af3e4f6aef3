"""CPU tests (no GPU): workspace sizing and argument checks of the normal equations wider than 111 columns (include/rdyn.h:
rdyn_gram_wide, rdyn_regressor_gram_wide, rdyn_identification_gram_wide).  Nothing here touches a device."""
import ctypes as C
import os

import pytest

from conftest import FIXTURES
from _cabi import RDYN_ERR_INVALID_ARGUMENT


def _long_xml(nj, seed):
    from rosdyn_amd.urdf_gen import generated_revolute_chain
    return generated_revolute_chain(nj, seed)


def test_gram_wide_workspace_by_width():
    from rosdyn_amd._lib import lib
    L = lib()
    for n_cols in (1, 111, 112, 200, 415):
        assert L.rdyn_gram_wide_workspace_bytes(n_cols) > 0, n_cols
    for n_cols in (0, -1, 416):
        assert L.rdyn_gram_wide_workspace_bytes(n_cols) == 0, n_cols
    # the narrow kernel's limit is unchanged
    assert L.rdyn_gram_workspace_bytes(112) == 0


@pytest.mark.parametrize("nj", [12, 14, 20, 32])
def test_regressor_gram_wide_workspace_for_many_input_joints(nj):
    from rosdyn_amd import Chain
    from rosdyn_amd._lib import lib
    L = lib()
    c = Chain(_long_xml(nj, 1000 + nj), "l0", "l%d" % nj)
    assert c.getActiveJointsNumber() == nj
    assert L.rdyn_regressor_gram_workspace_bytes(c._h, 0) == 0          # the narrow call still stops at 111 columns
    w = L.rdyn_regressor_gram_wide_workspace_bytes(c._h, 0)
    assert w > 0
    # the default chunk: the larger of 16 384 samples and what keeps one image within 128 MiB
    image = max(16384, ((128 << 20) // (nj * (10 * nj + 1) * 8)) & ~63) * nj * (10 * nj + 1) * 8
    assert image <= w <= image + L.rdyn_gram_wide_workspace_bytes(10 * nj) + 4096
    assert L.rdyn_regressor_gram_wide_workspace_bytes(c._h, 64) < w    # the caller's chunk size sizes the image


def test_regressor_gram_wide_workspace_permuted_inputs_and_fixed_joints():
    from rosdyn_amd.urdf_gen import generated_long_chain
    from rosdyn_amd import Chain
    from rosdyn_amd._lib import lib
    c = Chain(generated_long_chain(20, 2020), "l0", "l20")
    assert c.setInputJointsName(["j13", "j0", "j9", "j4", "j16", "j1", "j7", "j19", "j3", "j10", "j6", "j12"])
    assert c.getActiveJointsNumber() == 12 and c.getJointsNumber() == 20
    assert lib().rdyn_regressor_gram_workspace_bytes(c._h, 0) == 0
    assert lib().rdyn_regressor_gram_wide_workspace_bytes(c._h, 0) > 0


def test_identification_gram_wide_workspace_ur_with_26_friction_models():
    from rosdyn_amd import Chain
    from rosdyn_amd._lib import lib
    from rosdyn_amd.components import FRICTION1, ComponentSet
    L = lib()
    ur6 = Chain(os.path.join(FIXTURES, "ur10_like.urdf"), "base_link", "wrist_3_link")
    comps = ComponentSet([dict(type=FRICTION1, joint=j % 6, min_velocity=1e-3, max_velocity=5.0, parameters=[1.0, 1.0]) for j in range(26)], 6)
    assert comps.columns == 52
    arr = C.cast(comps._arr, C.c_void_p)
    assert L.rdyn_identification_gram_workspace_bytes(ur6._h, arr, comps.n_comps) == 0   # 60 + 52 = 112 > 111: refused by the narrow call
    w = L.rdyn_identification_gram_wide_workspace_bytes(ur6._h, arr, comps.n_comps, 0)
    assert w > 0
    assert L.rdyn_identification_gram_wide_workspace_bytes(ur6._h, arr, comps.n_comps, 256) < w
    # a request the narrow call serves is handed to it: the same workspace
    six = ComponentSet([dict(type=FRICTION1, joint=j, min_velocity=1e-3, max_velocity=5.0, parameters=[1.0, 1.0]) for j in range(6)], 6)
    a6 = C.cast(six._arr, C.c_void_p)
    assert L.rdyn_identification_gram_wide_workspace_bytes(ur6._h, a6, 6, 0) == L.rdyn_identification_gram_workspace_bytes(ur6._h, a6, 6)
    assert L.rdyn_regressor_gram_wide_workspace_bytes(ur6._h, 0) == L.rdyn_regressor_gram_workspace_bytes(ur6._h, 0)


def test_wide_queries_and_calls_refuse_bad_arguments_before_the_device():
    from rosdyn_amd import Chain
    from rosdyn_amd._lib import Batch, lib
    L = lib()
    assert L.rdyn_regressor_gram_wide_workspace_bytes(None, 0) == 0
    assert L.rdyn_identification_gram_wide_workspace_bytes(None, None, 0, 0) == 0
    c = Chain(_long_xml(14, 1014), "l0", "l14")
    fake = 4096   # never dereferenced: the checks come first
    b = Batch(100, fake, fake, fake, 0, 0, None)
    need = L.rdyn_regressor_gram_wide_workspace_bytes(c._h, 0)
    assert L.rdyn_regressor_gram_wide(c._h, C.byref(b), None, None, fake, fake, 0, 0, fake, need) == RDYN_ERR_INVALID_ARGUMENT
    assert L.rdyn_regressor_gram_wide(c._h, C.byref(b), None, fake, fake, fake, 0, 0, fake, need - 1) == RDYN_ERR_INVALID_ARGUMENT
    assert L.rdyn_regressor_gram_wide(c._h, C.byref(b), None, fake, fake, fake, 0, 0, None, need) == RDYN_ERR_INVALID_ARGUMENT
    assert L.rdyn_identification_gram_wide(c._h, None, 0, C.byref(b), fake, None, fake, fake, 0, 0, fake, need) == RDYN_ERR_INVALID_ARGUMENT
    assert L.rdyn_identification_gram_wide(c._h, None, 0, C.byref(b), fake, fake, fake, fake, 0, 0, fake, 16) == RDYN_ERR_INVALID_ARGUMENT
    w = L.rdyn_gram_wide_workspace_bytes(200)
    assert L.rdyn_gram_wide(fake, 1000, 1000, 200, None, fake, None, None, 0, fake, w - 1, 0, None) == RDYN_ERR_INVALID_ARGUMENT
    assert L.rdyn_gram_wide(fake, 1000, 1000, 200, None, None, None, None, 0, fake, w, 0, None) == RDYN_ERR_INVALID_ARGUMENT
    assert L.rdyn_gram_wide(fake, 1000, 999, 200, None, fake, None, None, 0, fake, w, 0, None) == RDYN_ERR_INVALID_ARGUMENT
