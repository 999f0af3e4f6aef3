"""CPU tests (no GPU): argument checks, routing and workspace queries of rdyn_rollout_adjoint_feedback_parameters (include/rdyn.h).
Nothing here touches a device: every call either has no samples or fails its checks first."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import FIXTURES, ROOT
from _cabi import (CHUNKED, EULER, FAKE, RDYN_ERR_INVALID_ARGUMENT, RDYN_ERR_UNSUPPORTED, RDYN_OK, RK4, SWEPT, _adjoint_desc as _desc, _batch, _chain,
                   _comp, _comps, _ext)

WHO = b"rdyn_rollout_adjoint_feedback_parameters"


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


def _pg(gpi=FAKE, gcomp=None, accumulate=0):
    from rosdyn_amd._lib import ParameterGradient
    return ParameterGradient(gpi, gcomp, accumulate)


def _gext(gw=FAKE, step_stride=0):
    from rosdyn_amd._lib import ExtWrenchGradient
    g = ExtWrenchGradient()
    g.gw, g.step_stride = gw, step_stride
    return g


def _query(chain, d, comps, n_comps, ext, fb, N, chunk=0):
    from rosdyn_amd._lib import lib
    p = lambda s: C.byref(s) if s is not None else None
    return lib().rdyn_rollout_adjoint_feedback_parameters_workspace_bytes(chain._h, C.byref(d) if d is not None else None, comps, n_comps, p(ext),
                                                                          p(fb), N, chunk)


def _base_query(chain, d, comps, n_comps, N, chunk=0):
    from rosdyn_amd._lib import lib
    return lib().rdyn_rollout_adjoint_parameters_workspace_bytes(chain._h, C.byref(d), comps, n_comps, N, chunk)


PG = object()


def _adj(chain, N, fb, gfb=None, pg=PG, ext=None, gext=None, desc=True, comps=None, n_comps=0, chunk_samples=0, workspace=FAKE, workspace_bytes=None,
         q=FAKE, dq=FAKE, batch=True, layout=0, **kw):
    from rosdyn_amd._lib import lib
    b = _batch(N, q, dq, layout)
    d = _desc(chain.getActiveJointsNumber(), max(N, 0), **kw)
    p = lambda s: C.byref(s) if s is not None else None
    if pg is PG:
        pg = _pg()
    if workspace_bytes is None:
        workspace_bytes = _query(chain, d, comps, n_comps, ext, fb, max(N, 0), max(chunk_samples, 0))
    return lib().rdyn_rollout_adjoint_feedback_parameters(chain._h, C.byref(b) if batch else None, C.byref(d) if desc else None, comps, n_comps,
                                                          p(ext), p(gext), p(fb), p(gfb), p(pg), chunk_samples, workspace, workspace_bytes)


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
    assert ("size_t rdyn_rollout_adjoint_feedback_parameters_workspace_bytes(const rdyn_chain* chain, const rdyn_rollout_adjoint_desc* desc, "
            "const rdyn_component* comps, int n_comps, const rdyn_ext_wrenches* ext, const rdyn_feedback* fb, int64_t n_samples, "
            "int64_t chunk_samples);") in flat
    assert ("int rdyn_rollout_adjoint_feedback_parameters(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_adjoint_desc* desc, "
            "const rdyn_component* comps, int n_comps, const rdyn_ext_wrenches* ext, const rdyn_ext_wrench_gradient* gext, "
            "const rdyn_feedback* fb, const rdyn_feedback_gradient* gfb, const rdyn_parameter_gradient* pg, "
            "int64_t chunk_samples, void* workspace, size_t workspace_bytes);") in flat
    # after rdyn_rollout_adjoint_feedback, before the mixed-chain section; the order of the earlier declarations stays
    order = ["int rdyn_rollout_adjoint(", "int rdyn_rollout_adjoint_parameters(", "int rdyn_rollout_adjoint_ext(", "int rdyn_rollout_adjoint_feedback(",
             "size_t rdyn_rollout_adjoint_feedback_parameters_workspace_bytes(", "int rdyn_rollout_adjoint_feedback_parameters(", "---- mixed-chain batch"]
    at = [flat.index(s) for s in order]
    assert at == sorted(at)
    # the phrases other tests pin, and the sentence that named the gap
    assert "The adjoint of the chunked closed loop is the follow-up" in flat
    assert "A device-side reduction is deliberately out of scope" in flat
    assert "mode with wrenches is the follow-up" in flat
    assert "so are the parameter gradients of the closed loop" not in flat
    prose = re.sub(r"\s+\*\s+", " ", open(ROOT + "/include/rdyn.h").read())   # comment text with the line breaks of the block comments taken out
    assert "The law does not depend on the model, so there is no further term." in prose
    l = _lib.lib()
    for name, nargs in (("rdyn_rollout_adjoint_feedback_parameters", 13), ("rdyn_rollout_adjoint_feedback_parameters_workspace_bytes", 8)):
        assert getattr(l, name) is not None and len(_lib.SYMBOLS[name][1]) == nargs


@pytest.mark.parametrize("name", SWEPT + ["rev10", "ur10_public_long"])
def test_every_refusal_of_a_chain_swept_in_registers(name):
    chain = _long() if name == "ur10_public_long" else _chain(name)
    n, nj, N = chain.getActiveJointsNumber(), chain.getJointsNumber(), 7
    bad_joint = _comp(joint=n)
    # no samples
    for g in (None, _gfb(), _gfb(gref_step_stride=n * N, gu_traj=FAKE, gu_step_stride=n * N, accumulate=1)):
        for integrator in (EULER, RK4):
            for acc in (0, 1):
                assert _adj(chain, 0, _fb(), g, _pg(accumulate=acc), integrator=integrator) == RDYN_OK
                assert _adj(chain, 0, _fb(hold=0, gains_per_sample=1), g, _pg(None, FAKE, acc), layout=1, integrator=integrator) == RDYN_OK
    assert _adj(chain, 0, _fb(), _gfb(), workspace=None, workspace_bytes=0) == RDYN_OK
    # the parameter selection: the open-loop call's refusals
    for pg in (None, _pg(None, None)):
        for samples in (0, N):
            assert _adj(chain, samples, _fb(), _gfb(), pg) == RDYN_ERR_INVALID_ARGUMENT and WHO in _err() and b"gpi" in _err()
    for acc in (-1, 2):
        assert _adj(chain, N, _fb(), _gfb(), _pg(accumulate=acc)) == RDYN_ERR_INVALID_ARGUMENT and WHO in _err() and b"accumulate" in _err()
    # the law: rdyn_rollout_feedback's refusals
    for kw in ({"q_ref": None}, {"kp": None}, {"ref_step_stride": -1}, {"ref_step_stride": n * N - 1}, {"ref_step_stride": 1}, {"hold": 2},
               {"hold": -1}, {"gains_per_sample": 2}):
        assert _adj(chain, N, _fb(**kw), _gfb()) == RDYN_ERR_INVALID_ARGUMENT, kw
        assert WHO in _err()
    # the law's gradient selection
    assert _adj(chain, N, _fb(kd=None), _gfb(gdq_ref=None)) == RDYN_ERR_INVALID_ARGUMENT and WHO in _err() and b"without a velocity gain" in _err()
    assert _adj(chain, N, _fb(kd=None), _gfb(gkd=None)) == RDYN_ERR_INVALID_ARGUMENT and b"without a velocity gain" in _err()
    assert _adj(chain, N, _fb(tau_limit=None), _gfb()) == RDYN_ERR_INVALID_ARGUMENT and WHO in _err() and b"glim without limits" in _err()
    for stride in (-1, 1, n * N - 1):
        assert _adj(chain, N, _fb(), _gfb(gref_step_stride=stride)) == RDYN_ERR_INVALID_ARGUMENT and WHO in _err() and b"gref_step_stride" in _err()
    for stride in (-1, 0, n * N - 1):
        assert _adj(chain, N, _fb(), _gfb(gu_traj=FAKE, gu_step_stride=stride)) == RDYN_ERR_INVALID_ARGUMENT and WHO in _err() and b"gu_traj" in _err()
    for acc in (-1, 2):
        assert _adj(chain, N, _fb(), _gfb(accumulate=acc)) == RDYN_ERR_INVALID_ARGUMENT and WHO in _err() and b"accumulate" in _err()
    # the two accumulate flags are independent: each value of one passes with each value of the other (what is refused next is the component list)
    for a in (0, 1):
        for b in (0, 1):
            assert _adj(chain, N, _fb(), _gfb(accumulate=a), _pg(accumulate=b), comps=C.addressof(bad_joint), n_comps=1) == RDYN_ERR_INVALID_ARGUMENT
            assert b"component" in _err()   # (the component-list text is shared by every dynamics call and names none of them)
    # "every output NULL" does not apply with gpi or gcomp: gq0, gdq0, gtau and the law's gradients may all be null
    nothing = dict(gq_ref=None, gdq_ref=None, gkp=None, gkd=None, glim=None)
    for g in (None, _gfb(**nothing)):
        for pg in (_pg(), _pg(None, FAKE)):
            assert _adj(chain, N, _fb(), g, pg, gq0=None, gdq0=None, gtau=None, comps=C.addressof(bad_joint), n_comps=1) == RDYN_ERR_INVALID_ARGUMENT
            assert b"component" in _err() and b"every output" not in _err()
    # every argument error of rdyn_rollout_adjoint
    for kw in ({"desc": False}, {"n_steps": -1}, {"dt": 0.0}, {"dt": float("nan")}, {"integrator": 2}, {"tau": None}, {"q_traj": None},
               {"traj_step_stride": n * N - 1}, {"gtraj_step_stride": n * N - 1}, {"gtau_step_stride": 1}, {"chunk_samples": -1},
               {"q": None}, {"dq": None}, {"batch": False}, {"layout": 5}, {"comps": None, "n_comps": 1}):
        assert _adj(chain, N, _fb(), _gfb(), workspace_bytes=1 << 40, **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
        assert _err()
    assert _adj(chain, -1, _fb(), _gfb()) == RDYN_ERR_INVALID_ARGUMENT
    assert _adj(chain, N, _fb(), _gfb(), PG, None, _gext()) == RDYN_ERR_INVALID_ARGUMENT and WHO in _err() and b"wrench gradient without external wrenches" in _err()
    # a workspace smaller than the query's answer
    assert _adj(chain, N, _fb(), _gfb(), workspace_bytes=_query(chain, _desc(n, N), None, 0, None, _fb(), N) - 1) == RDYN_ERR_INVALID_ARGUMENT
    assert WHO in _err() and b"workspace" in _err()
    assert _adj(chain, N, _fb(), _gfb(), workspace=None) == RDYN_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", SWEPT + ["rev10", "ur10_public_long"])
def test_the_workspace_is_the_accumulators_the_statuses_and_the_sums(name):
    chain = _long() if name == "ur10_public_long" else _chain(name)
    n = chain.getActiveJointsNumber()
    swept = n if name == "ur10_public_long" else chain.getJointsNumber()   # the reduced companion has one joint per input joint
    up = lambda x: (x + 255) // 256 * 256
    from rosdyn_amd._lib import lib
    for specs in ([], [(0, 0), (1, n - 1)]):
        comps = _comps(specs)
        K = lib().rdyn_components_columns(comps, len(specs)) if specs else 0
        cols = 10 * swept + K
        for N in (1, 7, 4096, 100000):
            for integrator in (EULER, RK4):
                for f in (_fb(), _fb(hold=0, gains_per_sample=1), None):
                    for chunk in (0, 1000):
                        d = _desc(n, N, integrator=integrator)
                        got = _query(chain, d, comps if specs else None, len(specs), None, f, N, chunk)
                        assert got == up(8 * N * cols) + up(4 * N) + up(8 * cols), (N, len(specs))
                        assert got == _base_query(chain, d, comps if specs else None, len(specs), N, chunk)
    d = _desc(n, 0)
    assert _query(chain, d, None, 0, None, _fb(), 0) == 0 and _query(chain, None, None, 0, None, _fb(), 7) == 0
    assert _query(chain, _desc(n, 7), None, 0, None, _fb(), 7, -1) == 0


@pytest.mark.parametrize("name", SWEPT + CHUNKED)
def test_without_a_law_the_call_and_the_query_are_the_open_loop_ones(name):
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 7
    for chunk in (0, 1000):
        for integrator in (EULER, RK4):
            for samples in (0, 7, 4096):
                d = _desc(n, samples, integrator=integrator)
                assert _query(chain, d, None, 0, None, None, samples, chunk) == _base_query(chain, d, None, 0, samples, chunk)
                assert _query(chain, d, None, 0, _ext(w=None), None, samples, chunk) == _base_query(chain, d, None, 0, samples, chunk)
    nothing = dict(gq_ref=None, gdq_ref=None, gkp=None, gkd=None, glim=None)
    # (the open-loop call refuses the chunked chains before it looks at the number of samples)
    served = RDYN_ERR_UNSUPPORTED if name in CHUNKED else RDYN_OK
    assert _adj(chain, 0, None) == served and _adj(chain, 0, None, _gfb(accumulate=7, gref_step_stride=-2, **nothing)) == served
    assert _adj(chain, 0, None, None, PG, _ext(w=None)) == served
    # the refusals are the open-loop call's, under its name
    assert _adj(chain, N, None, dt=0.0, workspace_bytes=1 << 40) == RDYN_ERR_INVALID_ARGUMENT and b"rdyn_rollout_adjoint_parameters:" in _err()
    assert _adj(chain, N, None, None, None) == RDYN_ERR_INVALID_ARGUMENT and b"rdyn_rollout_adjoint_parameters:" in _err()
    if name in CHUNKED:
        assert _adj(chain, N, None) == RDYN_ERR_UNSUPPORTED and b"rdyn_rollout_adjoint_parameters:" in _err() and b"rdyn_rollout_adjoint serves them" in _err()
    # a gradient with respect to a law that is not there
    for samples in (0, N):
        for g in (_gfb(), _gfb(**dict(nothing, gkp=FAKE)), _gfb(gu_traj=FAKE, **nothing)):
            assert _adj(chain, samples, None, g) == RDYN_ERR_INVALID_ARGUMENT and WHO in _err() and b"feedback gradient without a feedback law" in _err()
        assert _adj(chain, samples, None, None, PG, None, _gext()) == RDYN_ERR_INVALID_ARGUMENT and b"wrench gradient without external wrenches" in _err()


@pytest.mark.parametrize("name", SWEPT + ["rev10", "rev14", "ur10_public_long"])
def test_wrenches_are_unsupported_and_the_message_names_the_follow_up(name):
    chain = _long() if name == "ur10_public_long" else _chain(name)
    n, nj, N = chain.getActiveJointsNumber(), chain.getJointsNumber(), 7
    for x in (_ext(), _ext(link=nj), _ext(step_stride=6 * (nj + 1) * N)):
        for f in (_fb(), None):
            for samples in (N, 0):
                assert _adj(chain, samples, f, _gfb() if f is not None else None, PG, x, _gext(None)) == RDYN_ERR_UNSUPPORTED
                assert WHO in _err() and b"parameter gradients with external wrenches are the follow-up" in _err()
            assert _query(chain, _desc(n, N), None, 0, x, f, N) == 0
    # the argument errors still come first
    assert _adj(chain, N, _fb(kp=None), _gfb(), PG, _ext()) == RDYN_ERR_INVALID_ARGUMENT
    assert _adj(chain, N, _fb(), _gfb(), None, _ext()) == RDYN_ERR_INVALID_ARGUMENT
    assert _adj(chain, N, _fb(), _gfb(), PG, _ext(link=nj + 1)) == RDYN_ERR_INVALID_ARGUMENT and b"wrench link" in _err()


@pytest.mark.parametrize("name", CHUNKED + ["rev14"])
def test_the_chunked_chains_are_unsupported_with_the_wording_of_the_sibling(name):
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 7
    for samples in (N, 0):
        assert _adj(chain, samples, _fb(), _gfb()) == RDYN_ERR_UNSUPPORTED
        assert WHO in _err() and b"chunked route" in _err() and b"not served yet" in _err()
        assert b"the adjoint of the chunked closed loop is the follow-up" in _err()
    assert _query(chain, _desc(n, N), None, 0, None, _fb(), N) == 0
    # the argument errors still come first
    assert _adj(chain, N, _fb(kp=None), _gfb()) == RDYN_ERR_INVALID_ARGUMENT and _adj(chain, N, _fb(), _gfb(accumulate=3)) == RDYN_ERR_INVALID_ARGUMENT
    assert _adj(chain, N, _fb(), _gfb(), _pg(None, None)) == RDYN_ERR_INVALID_ARGUMENT and _adj(chain, N, _fb(), _gfb(), dt=0.0) == RDYN_ERR_INVALID_ARGUMENT


def test_python_keywords_exist():
    from rosdyn_amd import Chain, autograd
    p = inspect.signature(Chain.rolloutParameterAdjoint).parameters
    assert p["feedback"].default is None and p["want_feedback"].default == () and p["gu_traj"].default is None and p["sum_ref"].default is None
    assert p["accumulate"].default is False and list(p)[:7] == ["self", "q0", "Dq0", "tau", "dt", "q_traj", "Dq_traj"]
    s = inspect.signature(autograd.closed_loop_rollout).parameters
    assert list(s)[:6] == ["chain", "q0", "Dq0", "tau", "dt", "feedback"]
    assert all(k in s for k in ("integrator", "n_steps", "trajectory", "components", "layout")) and s["parameters"].default is None
    assert s["component_parameters"].default is None
    assert issubclass(autograd.RolloutFeedbackParametersFunction, __import__("torch").autograd.Function)
    assert "closed_loop_rollout" in autograd.__doc__ and "closed_loop_rollout" in autograd.__all__
