"""CPU tests (no GPU): argument checks and the workspace queries of rdyn_forward_dynamics_parameter_vjp and
rdyn_rollout_adjoint_parameters (include/rdyn.h).  Nothing here
touches a device: every call either has no samples or fails its checks first."""
import ctypes as C

import pytest

from _cabi import CHUNKED, FAKE, RDYN_ERR_INVALID_ARGUMENT, RDYN_OK, SWEPT, _chain, _comp


def _query(chain, N, comps=None, n_comps=0, chunk_samples=0):
    from rosdyn_amd._lib import lib
    return lib().rdyn_forward_dynamics_parameter_vjp_workspace_bytes(chain._h, comps, n_comps, N, chunk_samples)


def _pvjp(chain, N, q=FAKE, dq=FAKE, tau=FAKE, seed=FAKE, pi_bar=FAKE, comp_bar=FAKE, pi_sum=FAKE, comp_sum=FAKE, accumulate=0, tau_bar=FAKE,
          ddq=FAKE, status=FAKE, comps=None, n_comps=0, chunk_samples=0, workspace=FAKE, workspace_bytes=None, batch=True, layout=0):
    from rosdyn_amd._lib import Batch, lib
    b = Batch()
    b.n_samples, b.q, b.dq, b.layout, b.device = N, q, dq, layout, 0
    if workspace_bytes is None:
        workspace_bytes = _query(chain, max(N, 0), comps if n_comps > 0 else None, max(n_comps, 0), max(chunk_samples, 0))
    return lib().rdyn_forward_dynamics_parameter_vjp(chain._h, C.byref(b) if batch else None, comps, n_comps, tau, seed, pi_bar, comp_bar, pi_sum,
                                                     comp_sum, accumulate, tau_bar, ddq, status, chunk_samples, workspace, workspace_bytes)


@pytest.mark.parametrize("name", SWEPT + CHUNKED)
def test_no_samples_is_ok_and_every_listed_refusal(name):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    assert _pvjp(chain, 0) == RDYN_OK
    assert _pvjp(chain, 0, q=None, dq=None, tau=None, seed=None, pi_bar=None, comp_bar=None, pi_sum=None, comp_sum=None, tau_bar=None, ddq=None,
                 status=None, workspace=None, workspace_bytes=0) == RDYN_OK
    assert _pvjp(chain, 0, layout=1) == RDYN_OK
    one = _comp()
    bad_type, bad_joint = _comp(ctype=77), _comp(joint=n)
    refusals = [
        {"q": None}, {"dq": None}, {"batch": False},
        {"tau": None}, {"seed": None},
        {"pi_bar": None, "comp_bar": None, "pi_sum": None, "comp_sum": None, "tau_bar": None},
        {"accumulate": 2}, {"accumulate": -1},
        {"chunk_samples": -1},
        {"comps": None, "n_comps": 1}, {"comps": C.addressof(one), "n_comps": -1}, {"comps": C.addressof(one), "n_comps": 31},
        {"comps": C.addressof(bad_type), "n_comps": 1}, {"comps": C.addressof(bad_joint), "n_comps": 1},
    ]
    for kw in refusals:
        assert _pvjp(chain, 7, **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
        assert lib().rdyn_last_error()
    assert _pvjp(chain, -1) == RDYN_ERR_INVALID_ARGUMENT
    assert _pvjp(chain, 7, layout=5) == RDYN_ERR_INVALID_ARGUMENT
    assert _pvjp(chain, 0, chunk_samples=-1) == RDYN_ERR_INVALID_ARGUMENT
    assert _pvjp(chain, 0, accumulate=3) == RDYN_ERR_INVALID_ARGUMENT
    # every output is optional
    assert _pvjp(chain, 0, ddq=None, status=None, tau_bar=None, pi_bar=None, comp_bar=None, comp_sum=None) == RDYN_OK
    assert lib().rdyn_forward_dynamics_parameter_vjp(None, None, None, 0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0, FAKE, FAKE, FAKE, 0, FAKE,
                                                     1 << 30) == RDYN_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", SWEPT + ["rev10"])
def test_the_workspace_holds_one_partial_per_wave_and_the_total(name):
    chain = _chain(name)
    nj = chain.getJointsNumber()
    one = _comp(ctype=1)   # three columns
    assert _query(chain, 0) == 0 and _query(chain, 64, chunk_samples=-1) == 0
    for N in (1, 64, 65, 4096, 1 << 20):
        waves = (N + 63) // 64
        for comps, n_comps, K in ((None, 0, 0), (C.addressof(one), 1, 3)):
            need = _query(chain, N, comps, n_comps)
            cols = 10 * nj + K
            assert (waves + 1) * cols * 8 <= need <= (waves + 1) * cols * 8 + 512
    # a sum needs the workspace, the rows alone do not (the refusal comes before any device work)
    need = _query(chain, 7)
    assert _pvjp(chain, 7, workspace_bytes=need - 1) == RDYN_ERR_INVALID_ARGUMENT
    assert _pvjp(chain, 7, workspace=None, workspace_bytes=need) == RDYN_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", CHUNKED)
def test_the_workspace_of_the_chunked_route(name):
    """the product's own workspace, tau_bar, ddq and the status of the batch, one chunk's image, the rows and the totals; always needed"""
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n, P = chain.getActiveJointsNumber(), 10 * chain.getJointsNumber()
    assert n > 10
    one = _comp(ctype=1)   # three columns
    for N in (7, 5000):
        for comps, n_comps, K in ((None, 0, 0), (C.addressof(one), 1, 3)):
            sizes = [_query(chain, N, comps, n_comps, chunk) for chunk in (64, 1000, 16384)]
            assert sizes == sorted(sizes) and sizes[0] > 0
            for chunk, s in zip((64, 1000, 16384), sizes):
                image = min(chunk, (N + 63) // 64 * 64) * n * (P + K + 1) * 8
                assert s >= lib().rdyn_forward_dynamics_vjp_workspace_bytes(chain._h, chunk) + 2 * n * N * 8 + 4 * N + image + (P + K) * (N + 1) * 8
    assert _query(chain, 0) == 0 and _query(chain, 64, chunk_samples=-1) == 0
    need = _query(chain, 7, chunk_samples=1000)
    for kw in ({}, {"pi_sum": None, "comp_sum": None}):   # with and without a sum
        assert _pvjp(chain, 7, chunk_samples=1000, workspace_bytes=need - 1, **kw) == RDYN_ERR_INVALID_ARGUMENT
        assert _pvjp(chain, 7, chunk_samples=1000, workspace=None, workspace_bytes=need, **kw) == RDYN_ERR_INVALID_ARGUMENT
    assert _pvjp(chain, 0, workspace=None, workspace_bytes=0) == RDYN_OK


# ---- rdyn_rollout_adjoint_parameters --------------------------------------------------------------------------------
def _padj_query(chain, d, N, comps=None, n_comps=0, chunk_samples=0):
    from rosdyn_amd._lib import lib
    return lib().rdyn_rollout_adjoint_parameters_workspace_bytes(chain._h, C.byref(d), comps, n_comps, N, chunk_samples)


def _padj(chain, N, desc=True, comps=None, n_comps=0, chunk_samples=0, workspace=FAKE, workspace_bytes=None, q=FAKE, dq=FAKE, batch=True, layout=0,
          pg=True, gpi=FAKE, gcomp=FAKE, accumulate=0, **kw):
    from rosdyn_amd._lib import Batch, ParameterGradient, lib
    from _cabi import _adjoint_desc as _desc
    b = Batch()
    b.n_samples, b.q, b.dq, b.layout, b.device = N, q, dq, layout, 0
    d = _desc(chain.getActiveJointsNumber(), max(N, 0), **kw)
    if workspace_bytes is None:
        workspace_bytes = _padj_query(chain, d, max(N, 0), comps if n_comps > 0 else None, max(n_comps, 0), max(chunk_samples, 0))
    g = ParameterGradient(gpi, gcomp, accumulate)
    return lib().rdyn_rollout_adjoint_parameters(chain._h, C.byref(b) if batch else None, C.byref(d) if desc else None, comps, n_comps,
                                                 C.byref(g) if pg else None, chunk_samples, workspace, workspace_bytes)


@pytest.mark.parametrize("name", SWEPT + ["rev10"])
def test_rollout_call_no_samples_is_ok_and_every_listed_refusal(name):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 7
    assert _padj(chain, 0) == RDYN_OK
    assert _padj(chain, 0, q=None, dq=None, gq0=None, gdq0=None, gtau=None, status=None, gq_end=None, gdq_end=None, gq_traj=None, gdq_traj=None,
                 workspace=None, workspace_bytes=0) == RDYN_OK
    assert _padj(chain, 0, layout=1, integrator=0, gcomp=None) == RDYN_OK and _padj(chain, 0, gpi=None, accumulate=1) == RDYN_OK
    one = _comp()
    bad_type, bad_joint = _comp(ctype=77), _comp(joint=n)
    refusals = [
        {"pg": False}, {"gpi": None, "gcomp": None}, {"accumulate": 2}, {"accumulate": -1},     # what this call adds
        {"desc": False},                                                                         # ... and rdyn_rollout_adjoint's
        {"n_steps": -1}, {"dt": 0.0}, {"dt": float("inf")}, {"dt": float("nan")}, {"integrator": 2}, {"integrator": -1},
        {"tau": None},
        {"q_traj": None}, {"dq_traj": None}, {"q_traj": None, "n_steps": 2},
        {"traj_step_stride": n * N - 1}, {"traj_step_stride": 0},
        {"gtraj_step_stride": n * N - 1}, {"gtraj_step_stride": 0, "gq_traj": None},
        {"gtau_step_stride": n * N - 1}, {"gtau_step_stride": 1}, {"gtau_step_stride": -n * N},
        {"comps": None, "n_comps": 1}, {"comps": C.addressof(one), "n_comps": -1}, {"comps": C.addressof(one), "n_comps": 31},
        {"comps": C.addressof(bad_type), "n_comps": 1}, {"comps": C.addressof(bad_joint), "n_comps": 1},
        {"chunk_samples": -1},
        {"q": None}, {"dq": None}, {"batch": False},
        {"workspace": None}, {"workspace_bytes": 0},
    ]
    for kw in refusals:
        assert _padj(chain, N, **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
        assert lib().rdyn_last_error()
    assert _padj(chain, -1) == RDYN_ERR_INVALID_ARGUMENT and _padj(chain, N, layout=5) == RDYN_ERR_INVALID_ARGUMENT
    assert _padj(chain, 0, pg=False) == RDYN_ERR_INVALID_ARGUMENT and _padj(chain, 0, gpi=None, gcomp=None) == RDYN_ERR_INVALID_ARGUMENT
    # gq0, gdq0 and gtau may all be null here
    assert _padj(chain, 0, gq0=None, gdq0=None, gtau=None) == RDYN_OK
    # the workspace: the lanes' accumulators, one status word per sample, the column sums
    from _cabi import _adjoint_desc as _desc
    nj = chain.getJointsNumber()
    three = _comp(ctype=1)
    for M in (1, 65, 4096):
        for comps, n_comps, K in ((None, 0, 0), (C.addressof(three), 1, 3)):
            need = _padj_query(chain, _desc(n, M), M, comps, n_comps)
            low = (10 * nj + K) * (M + 1) * 8 + 4 * M
            assert low <= need <= low + 768
    assert _padj_query(chain, _desc(n, 0), 0) == 0 and _padj_query(chain, _desc(n, 64), 64, chunk_samples=-1) == 0


@pytest.mark.parametrize("name", CHUNKED)
def test_rollout_call_refuses_chains_the_kernels_do_not_sweep(name):
    """RDYN_ERR_UNSUPPORTED, with no device needed; the argument errors of the descriptor still come first, no samples is still RDYN_OK"""
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    assert chain.getActiveJointsNumber() > 10
    for integrator in (0, 1):
        assert _padj(chain, 7, integrator=integrator) == 5
        assert b"input joints" in lib().rdyn_last_error()
    assert _padj(chain, 7, pg=False) == RDYN_ERR_INVALID_ARGUMENT and _padj(chain, 7, dt=0.0) == RDYN_ERR_INVALID_ARGUMENT
    assert _padj(chain, 7, desc=False) == RDYN_ERR_INVALID_ARGUMENT


def test_python_bindings_exist():
    from rosdyn_amd import Chain, autograd
    from rosdyn_amd.components import ComponentSet
    for name in ("withParameters", "getJointAccelerationParameterVjp", "rolloutParameterAdjoint"):
        assert callable(getattr(Chain, name))
    assert callable(ComponentSet.withParameters)
    assert autograd.JointAccelerationParametersFunction and autograd.RolloutParametersFunction
    cs = ComponentSet([dict(type=1, joint=0, min_velocity=0.1, max_velocity=2.0, parameters=[1.0, 2.0, 3.0]),
                       dict(type=2, joint=1, parameters=[4.0, 5.0])], 6)
    other = cs.withParameters([9.0, 8.0, 7.0, 6.0, 5.0])
    assert other.getNominalParameters() == [9.0, 8.0, 7.0, 6.0, 5.0] and cs.getNominalParameters() == [1.0, 2.0, 3.0, 4.0, 5.0]
    assert other.columns == 5 and other._arr[0].min_velocity == 0.1 and other._arr[1].joint == 1
    with pytest.raises(ValueError):
        cs.withParameters([1.0])
