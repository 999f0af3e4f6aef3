from _cabi import RDYN_ERR_INVALID_ARGUMENT, RDYN_ERR_UNSUPPORTED

"""CPU tests (no GPU): workspace sizing and argument checks of the R factor wider than 112 columns (include/rdyn.h: rdyn_tsqr_wide,
rdyn_tsqr_wide_last_report).  Nothing here touches a device."""


def test_tsqr_wide_workspace_by_width():
    from rosdyn_amd._lib import lib
    L = lib()
    sizes = [L.rdyn_tsqr_wide_workspace_bytes(n1) for n1 in (113, 200, 321, 415, 416)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes)
    # the workspace holds one row chunk of Q: at least 16 384 rows of n1 columns
    assert sizes[-1] >= 16384 * 416 * 8
    for n1 in (0, -1, 417, 1000):
        assert L.rdyn_tsqr_wide_workspace_bytes(n1) == 0, n1
    # widths rdyn_tsqr serves are handed to it: its workspace size
    for n1 in (1, 2, 64, 96, 112):
        assert L.rdyn_tsqr_wide_workspace_bytes(n1) == L.rdyn_tsqr_workspace_bytes(n1) > 0, n1
    # the narrow limit is unchanged
    assert L.rdyn_tsqr_workspace_bytes(113) == 0


def test_tsqr_wide_refuses_bad_arguments_before_the_device():
    from rosdyn_amd._lib import lib
    L = lib()
    fake = 4096   # never dereferenced: the checks come first
    w = L.rdyn_tsqr_wide_workspace_bytes(201)
    ok = (fake, 1000, 1000, 200, fake, fake, 0, fake, w, 0, None)

    def call(**kw):
        names = ("A", "rows", "lda", "n_cols", "b", "R", "acc", "ws", "wsb", "dev", "stream")
        args = dict(zip(names, ok))
        args.update(kw)
        return L.rdyn_tsqr_wide(*(args[n] for n in names))

    assert call(A=None) == RDYN_ERR_INVALID_ARGUMENT
    assert call(R=None) == RDYN_ERR_INVALID_ARGUMENT
    assert call(ws=None) == RDYN_ERR_INVALID_ARGUMENT
    assert call(wsb=w - 1) == RDYN_ERR_INVALID_ARGUMENT
    assert call(lda=999) == RDYN_ERR_INVALID_ARGUMENT
    assert call(rows=-1) == RDYN_ERR_INVALID_ARGUMENT
    assert call(n_cols=0) == RDYN_ERR_INVALID_ARGUMENT
    # past the wide limit: unsupported (with and without the right-hand side)
    assert call(n_cols=416) == RDYN_ERR_UNSUPPORTED
    assert call(n_cols=417, b=None) == RDYN_ERR_UNSUPPORTED
    assert L.rdyn_tsqr_wide_last_report(201, None, 0, None, fake) == RDYN_ERR_INVALID_ARGUMENT
    assert L.rdyn_tsqr_wide_last_report(201, fake, 0, None, None) == RDYN_ERR_INVALID_ARGUMENT
    assert L.rdyn_tsqr_wide_last_report(500, fake, 0, None, fake) == RDYN_ERR_UNSUPPORTED


def test_tsqr_wide_report_of_a_narrow_width_is_route_0():
    import ctypes as C
    from rosdyn_amd._lib import RdynTsqrWideReport, lib
    rep = RdynTsqrWideReport()
    rep.route = 7
    assert lib().rdyn_tsqr_wide_last_report(50, 4096, 0, None, C.byref(rep)) == 0
    assert rep.route == 0 and rep.stage == 0 and tuple(rep.gamma) == (0.0, 0.0, 0.0)


def _rev(nj):
    from rosdyn_amd.urdf_gen import generated_revolute_chain
    from rosdyn_amd import Chain
    return Chain(generated_revolute_chain(nj, 1000 + nj), "l0", "l%d" % nj)


def test_regressor_tsqr_wide_workspace_for_many_input_joints():
    from rosdyn_amd._lib import lib
    L = lib()
    for nj in (12, 14, 20, 32):
        c = _rev(nj)
        assert L.rdyn_regressor_tsqr_workspace_bytes(c._h) == 0           # the narrow call stops at 112 columns
        w = L.rdyn_regressor_tsqr_wide_workspace_bytes(c._h, 0)
        assert w >= 16384 * nj * (10 * nj + 1) * 8, nj                    # at least one default chunk image
        assert 0 < L.rdyn_regressor_tsqr_wide_workspace_bytes(c._h, 96) < w
    assert L.rdyn_regressor_tsqr_wide_workspace_bytes(None, 0) == 0


def test_tsqr_wide_workspace_fixed_joints_components_and_hand_off():
    import ctypes as C
    import os
    from conftest import FIXTURES
    from rosdyn_amd.urdf_gen import generated_long_chain
    from rosdyn_amd import Chain
    from rosdyn_amd._lib import lib
    from rosdyn_amd.components import FRICTION1, ComponentSet
    L = lib()
    c = Chain(generated_long_chain(20, 2020), "l0", "l20")
    assert c.setInputJointsName(["j13", "j0", "j9", "j4", "j16", "j1", "j7", "j19", "j3", "j10", "j6", "j12"])
    assert L.rdyn_regressor_tsqr_workspace_bytes(c._h) == 0 and L.rdyn_regressor_tsqr_wide_workspace_bytes(c._h, 0) > 0
    ur6 = Chain(os.path.join(FIXTURES, "ur10_like.urdf"), "base_link", "wrist_3_link")
    comps = ComponentSet([dict(type=FRICTION1, joint=j % 6, min_velocity=1e-3, max_velocity=5.0, parameters=[1.0, 1.0]) for j in range(26)], 6)
    arr = C.cast(comps._arr, C.c_void_p)
    assert L.rdyn_identification_tsqr_workspace_bytes(ur6._h, arr, comps.n_comps) == 0
    assert L.rdyn_identification_tsqr_wide_workspace_bytes(ur6._h, arr, comps.n_comps, 0) > 0
    # served by the narrow call: its workspace size
    assert L.rdyn_regressor_tsqr_wide_workspace_bytes(ur6._h, 0) == L.rdyn_regressor_tsqr_workspace_bytes(ur6._h) > 0
    # past 416 columns: 0 (32 joints + 10 friction models = 341 columns; + 40 more = 421)
    c32 = _rev(32)
    many = ComponentSet([dict(type=FRICTION1, joint=j % 32, min_velocity=1e-3, max_velocity=5.0, parameters=[1.0, 1.0]) for j in range(50)], 32)
    assert L.rdyn_identification_tsqr_wide_workspace_bytes(c32._h, C.cast(many._arr, C.c_void_p), many.n_comps, 0) == 0


def test_chain_tsqr_wide_calls_refuse_bad_arguments_before_the_device():
    import ctypes as C
    from rosdyn_amd._lib import Batch, lib
    L = lib()
    c = _rev(14)
    fake = 4096
    b = Batch(100, fake, fake, fake, 0, 0, None)
    need = L.rdyn_regressor_tsqr_wide_workspace_bytes(c._h, 0)
    assert L.rdyn_regressor_tsqr_wide(c._h, C.byref(b), None, None, 0, 0, fake, need) == RDYN_ERR_INVALID_ARGUMENT
    assert L.rdyn_regressor_tsqr_wide(c._h, C.byref(b), None, fake, 0, 0, fake, need - 1) == RDYN_ERR_INVALID_ARGUMENT
    assert L.rdyn_regressor_tsqr_wide(c._h, C.byref(b), None, fake, 0, 0, None, need) == RDYN_ERR_INVALID_ARGUMENT
    assert L.rdyn_regressor_tsqr_wide(c._h, C.byref(b), None, fake, 0, -1, fake, need) == RDYN_ERR_INVALID_ARGUMENT
    assert L.rdyn_identification_tsqr_wide(c._h, None, 0, C.byref(b), fake, fake, 0, 0, fake, 16) == RDYN_ERR_INVALID_ARGUMENT
