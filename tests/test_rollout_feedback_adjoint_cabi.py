"""CPU tests (no GPU): argument checks, routing and workspace queries of rdyn_rollout_adjoint_feedback (include/rdyn.h).  Nothing here
touches a device: every call either has no samples or fails its checks first."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import FIXTURES, ROOT
from _cabi import (CHUNKED, EULER, FAKE, RDYN_ERR_INVALID_ARGUMENT, RDYN_ERR_UNSUPPORTED, RDYN_OK, RK4, SWEPT, _adj_query,
                   _adjoint_desc as _desc, _batch, _chain, _comp, _ext)


def _fb(**kw):
    from rosdyn_amd._lib import Feedback
    f = Feedback()
    f.q_ref, f.dq_ref, f.ref_step_stride, f.kp, f.kd, f.gains_per_sample, f.hold, f.tau_limit = FAKE, FAKE, 0, FAKE, FAKE, 0, 1, FAKE
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def _gfb(**kw):
    from rosdyn_amd._lib import FeedbackGradient
    g = FeedbackGradient()
    g.gq_ref, g.gdq_ref, g.gref_step_stride, g.gkp, g.gkd, g.glim, g.accumulate, g.gu_traj, g.gu_step_stride = FAKE, FAKE, 0, FAKE, FAKE, FAKE, 0, None, 0
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _gext(gw=FAKE, step_stride=0):
    from rosdyn_amd._lib import ExtWrenchGradient
    g = ExtWrenchGradient()
    g.gw, g.step_stride = gw, step_stride
    return g


def _adj(chain, N, fb, gfb=None, ext=None, gext=None, desc=True, comps=None, n_comps=0, chunk_samples=0, workspace=FAKE, workspace_bytes=None,
         q=FAKE, dq=FAKE, batch=True, layout=0, **kw):
    from rosdyn_amd._lib import lib
    b = _batch(N, q, dq, layout)
    d = _desc(chain.getActiveJointsNumber(), max(N, 0), **kw)
    p = lambda s: C.byref(s) if s is not None else None
    if workspace_bytes is None:
        workspace_bytes = lib().rdyn_rollout_adjoint_feedback_workspace_bytes(chain._h, C.byref(d), p(ext), p(fb), max(N, 0), max(chunk_samples, 0))
    return lib().rdyn_rollout_adjoint_feedback(chain._h, C.byref(b) if batch else None, C.byref(d) if desc else None, comps, n_comps, p(ext),
                                               p(gext), p(fb), p(gfb), chunk_samples, workspace, workspace_bytes)


def _err():
    from rosdyn_amd._lib import lib
    return lib().rdyn_last_error()


def _long():
    from rosdyn_amd import Chain
    chain = Chain(os.path.join(FIXTURES, "ur10_public_long.urdf"), "base_link", "tcp")
    assert chain.getJointsNumber() > 10 and chain.getActiveJointsNumber() <= 10
    return chain


def test_the_symbols_exist_with_the_documented_signatures():
    from rosdyn_amd import _lib
    flat = re.sub(r"\s+", " ", open(ROOT + "/include/rdyn.h").read())
    assert ("int rdyn_rollout_adjoint_feedback(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_adjoint_desc* desc, "
            "const rdyn_component* comps, int n_comps, const rdyn_ext_wrenches* ext, const rdyn_ext_wrench_gradient* gext, "
            "const rdyn_feedback* fb, const rdyn_feedback_gradient* gfb, int64_t chunk_samples, void* workspace, size_t workspace_bytes);") in flat
    assert "size_t rdyn_rollout_adjoint_feedback_workspace_bytes(" in flat
    assert flat.index("int rdyn_rollout_adjoint_ext(") < flat.index("size_t rdyn_rollout_adjoint_feedback_workspace_bytes(")
    assert "does not transpose the feedback law" not in flat and "rdyn_rollout_adjoint_feedback (below) is the transpose of this call" in flat and"The adjoint of the chunked closed loop is the follow-up" in flat
    assert "A device-side reduction is deliberately out of scope" in flat
    l = _lib.lib()
    for name, nargs in (("rdyn_rollout_adjoint_feedback", 12), ("rdyn_rollout_adjoint_feedback_workspace_bytes", 6)):
        assert getattr(l, name) is not None and len(_lib.SYMBOLS[name][1]) == nargs
    assert C.sizeof(_lib.FeedbackGradient) == 72


@pytest.mark.parametrize("name", SWEPT + ["rev10", "ur10_public_long"])
def test_every_refusal_of_a_chain_swept_in_registers(name):
    from rosdyn_amd._lib import lib
    chain = _long() if name == "ur10_public_long" else _chain(name)
    n, nj, N = chain.getActiveJointsNumber(), chain.getJointsNumber(), 7
    L = nj + 1
    bad_joint = _comp(joint=n)
    exts = (None,) if name == "ur10_public_long" else (None, _ext(), _ext(link=nj, step_stride=6 * N))
    # no samples
    for x in exts:
        for g in (None, _gfb(), _gfb(gref_step_stride=n * N, gu_traj=FAKE, gu_step_stride=n * N, accumulate=1)):
            for integrator in (EULER, RK4):
                assert _adj(chain, 0, _fb(), g, x, integrator=integrator) == RDYN_OK
                assert _adj(chain, 0, _fb(hold=0, gains_per_sample=1), g, x, layout=1, integrator=integrator) == RDYN_OK
    for x in exts:
        gx = _gext() if x is not None else None
        # the law: rdyn_rollout_feedback's refusals
        for kw in ({"q_ref": None}, {"kp": None}, {"ref_step_stride": -1}, {"ref_step_stride": n * N - 1}, {"ref_step_stride": 1}, {"hold": 2},
                   {"hold": -1}, {"gains_per_sample": 2}):
            assert _adj(chain, N, _fb(**kw), _gfb(), x, gx) == RDYN_ERR_INVALID_ARGUMENT, kw
            assert b"rdyn_rollout_adjoint_feedback" in _err()
        # the gradient selection
        assert _adj(chain, N, _fb(kd=None), _gfb(gdq_ref=None), x, gx) == RDYN_ERR_INVALID_ARGUMENT and b"without a velocity gain" in _err()
        assert _adj(chain, N, _fb(kd=None), _gfb(gkd=None), x, gx) == RDYN_ERR_INVALID_ARGUMENT and b"without a velocity gain" in _err()
        assert _adj(chain, N, _fb(tau_limit=None), _gfb(), x, gx) == RDYN_ERR_INVALID_ARGUMENT and b"glim without limits" in _err()
        for stride in (-1, 1, n * N - 1):
            assert _adj(chain, N, _fb(), _gfb(gref_step_stride=stride), x, gx) == RDYN_ERR_INVALID_ARGUMENT and b"gref_step_stride" in _err()
        for stride in (-1, 0, n * N - 1):
            assert _adj(chain, N, _fb(), _gfb(gu_traj=FAKE, gu_step_stride=stride), x, gx) == RDYN_ERR_INVALID_ARGUMENT and b"gu_traj" in _err()
        for acc in (-1, 2):
            assert _adj(chain, N, _fb(), _gfb(accumulate=acc), x, gx) == RDYN_ERR_INVALID_ARGUMENT and b"accumulate" in _err()
        # every output null with samples; any one of them is enough (what is refused next is the component list)
        nothing = dict(gq_ref=None, gdq_ref=None, gkp=None, gkd=None, glim=None)
        for g in (None, _gfb(**nothing), _gfb(gu_traj=FAKE, gu_step_stride=n * N, **nothing)):
            assert _adj(chain, N, _fb(), g, x, _gext(None) if x is not None else None, gq0=None, gdq0=None, gtau=None) == RDYN_ERR_INVALID_ARGUMENT
            assert b"every output" in _err()
        for one in nothing:
            g = _gfb(**dict(nothing, **{one: FAKE}))
            assert _adj(chain, N, _fb(), g, x, None, gq0=None, gdq0=None, gtau=None, comps=C.addressof(bad_joint), n_comps=1) == RDYN_ERR_INVALID_ARGUMENT
            assert b"component" in _err()
        # the smallest valid strides pass; without gq_ref / gdq_ref and without gu_traj their strides are not read
        for g in (_gfb(gref_step_stride=n * N, gu_traj=FAKE, gu_step_stride=n * N), _gfb(gq_ref=None, gdq_ref=None, gref_step_stride=-3, gu_step_stride=-3)):
            assert _adj(chain, N, _fb(ref_step_stride=n * N), g, x, gx, comps=C.addressof(bad_joint), n_comps=1) == RDYN_ERR_INVALID_ARGUMENT
            assert b"component" in _err()
        # every argument error of rdyn_rollout_adjoint_ext
        for kw in ({"desc": False}, {"n_steps": -1}, {"dt": 0.0}, {"dt": float("nan")}, {"integrator": 2}, {"tau": None}, {"q_traj": None},
                   {"traj_step_stride": n * N - 1}, {"gtraj_step_stride": n * N - 1}, {"gtau_step_stride": 1}, {"chunk_samples": -1},
                   {"q": None}, {"dq": None}, {"batch": False}, {"layout": 5}, {"comps": None, "n_comps": 1}):
            assert _adj(chain, N, _fb(), _gfb(), x, gx, **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
            assert _err()
        assert _adj(chain, -1, _fb(), _gfb(), x, gx) == RDYN_ERR_INVALID_ARGUMENT
    if name != "ur10_public_long":
        assert _adj(chain, N, _fb(), _gfb(), _ext(link=nj + 1)) == RDYN_ERR_INVALID_ARGUMENT and b"wrench link" in _err()
        assert _adj(chain, N, _fb(), _gfb(), _ext(step_stride=6 * L * N - 1)) == RDYN_ERR_INVALID_ARGUMENT and b"wrench step_stride" in _err()
        assert _adj(chain, N, _fb(), _gfb(), _ext(), _gext(step_stride=1)) == RDYN_ERR_INVALID_ARGUMENT and b"wrench-gradient step_stride" in _err()
    assert _adj(chain, N, _fb(), _gfb(), None, _gext()) == RDYN_ERR_INVALID_ARGUMENT and b"wrench gradient without external wrenches" in _err()
    # one launch, no workspace: the query is 0 and a null workspace is accepted
    for x in exts:
        for chunk in (0, 1000):
            for integrator in (EULER, RK4):
                d = _desc(n, N, integrator=integrator)
                f = _fb()
                assert lib().rdyn_rollout_adjoint_feedback_workspace_bytes(chain._h, C.byref(d), C.byref(x) if x is not None else None, C.byref(f), N, chunk) == 0
        assert _adj(chain, 0, _fb(), _gfb(), x, workspace=None, workspace_bytes=0) == RDYN_OK


@pytest.mark.parametrize("name", SWEPT + CHUNKED)
def test_without_a_law_the_call_and_the_query_are_the_base_ones(name):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 7
    for chunk in (0, 1000, 20000):
        for integrator in (EULER, RK4):
            for samples in (0, 7, 4096):
                d = _desc(n, samples, integrator=integrator)
                assert lib().rdyn_rollout_adjoint_feedback_workspace_bytes(chain._h, C.byref(d), None, None, samples, chunk) == _adj_query(chain, d, samples, chunk)
    nothing = dict(gq_ref=None, gdq_ref=None, gkp=None, gkd=None, glim=None)
    assert _adj(chain, 0, None) == RDYN_OK and _adj(chain, 0, None, _gfb(accumulate=7, gref_step_stride=-2, **nothing)) == RDYN_OK
    assert _adj(chain, N, None, dt=0.0) == RDYN_ERR_INVALID_ARGUMENT and b"rdyn_rollout_adjoint:" in _err()
    # a gradient with respect to a law that is not there
    for samples in (0, N):
        for g in (_gfb(), _gfb(**dict(nothing, gkp=FAKE)), _gfb(gu_traj=FAKE, **nothing)):
            assert _adj(chain, samples, None, g) == RDYN_ERR_INVALID_ARGUMENT and b"feedback gradient without a feedback law" in _err()
        assert _adj(chain, samples, None, None, None, _gext()) == RDYN_ERR_INVALID_ARGUMENT and b"wrench gradient without external wrenches" in _err()


@pytest.mark.parametrize("name", CHUNKED + ["rev14", "ur10_public_long"])
def test_the_chunked_chains_are_unsupported_and_the_message_says_so(name):
    chain = _long() if name == "ur10_public_long" else _chain(name)
    nj, N = chain.getJointsNumber(), 7
    for x in ((_ext(), _ext(link=nj)) if name == "ur10_public_long" else (None, _ext(), _ext(link=nj))):
        for samples in (N, 0):
            assert _adj(chain, samples, _fb(), _gfb(), x) == RDYN_ERR_UNSUPPORTED
            assert b"rdyn_rollout_adjoint_feedback" in _err() and b"chunked route" in _err() and b"not served yet" in _err()
    # the argument errors still come first
    assert _adj(chain, N, _fb(kp=None), _gfb()) == RDYN_ERR_INVALID_ARGUMENT and _adj(chain, N, _fb(), _gfb(accumulate=3)) == RDYN_ERR_INVALID_ARGUMENT
    assert _adj(chain, N, _fb(), _gfb(), dt=0.0) == RDYN_ERR_INVALID_ARGUMENT
    # without a law these chains are served as before
    assert _adj(chain, 0, None) == RDYN_OK


def test_python_keywords_exist():
    from rosdyn_amd import Chain, autograd
    p = inspect.signature(Chain.rolloutAdjoint).parameters
    assert p["feedback"].default is None and p["want_feedback"].default == () and p["gu_traj"].default is None and p["accumulate"].default is False
    assert inspect.signature(autograd.rollout).parameters["feedback"].default is None
    assert issubclass(autograd.RolloutFeedbackFunction, __import__("torch").autograd.Function)
    assert "does not serve the closed loop" not in autograd.__doc__
