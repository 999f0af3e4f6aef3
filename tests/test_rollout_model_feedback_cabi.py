"""CPU tests (no GPU): the symbols, argument checks, routing and workspace queries of rdyn_rollout_model_feedback (include/rdyn.h) and the
Python surface.  Nothing touches a device: every call either has no samples or fails its checks first."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import FIXTURES, ROOT
from _cabi import (CHUNKS, EULER, FAKE, INTEGRATOR_CODES, RDYN_ERR_INVALID_ARGUMENT, RDYN_ERR_UNSUPPORTED, RDYN_OK, SAMPLES, SWEPT, _batch, _chain,
                   _comps, _ext, _rollout_desc as _desc)
from _chains import FILES
from _components import FRICTION1, SPRING

WHO = b"rdyn_rollout_model_feedback"
GC_LAW, CT_LAW = 1, 2


def _fb(**kw):
    from rosdyn_amd._lib import Feedback
    f = Feedback()
    f.q_ref, f.dq_ref, f.ref_step_stride, f.kp, f.kd, f.gains_per_sample, f.hold, f.tau_limit, f.tau_traj = FAKE, FAKE, 0, FAKE, FAKE, 0, 1, FAKE, None
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def _mfb(model, law=CT_LAW, ddq_ref=None):
    from rosdyn_amd._lib import ModelFeedback
    m = ModelFeedback()
    m.model, m.law, m.ddq_ref = (model._h if model is not None else None), law, ddq_ref
    return m


def _ref(x):
    return C.byref(x) if x is not None else None


def _need(chain, d, ext, fb, mfb, N, chunk=0):
    from rosdyn_amd._lib import lib
    return lib().rdyn_rollout_model_feedback_workspace_bytes(chain._h, C.byref(d), _ref(ext), _ref(fb), _ref(mfb), N, chunk)


def _call(chain, N, fb, mfb, ext=None, comps=None, n_comps=0, desc=True, chunk_samples=0, workspace=FAKE, workspace_bytes=None, q=FAKE, dq=FAKE,
          batch=True, layout=0, **kw):
    from rosdyn_amd._lib import lib
    b = _batch(N, q, dq, layout)
    d = _desc(chain.getActiveJointsNumber(), max(N, 0), **kw)
    if workspace_bytes is None:
        workspace_bytes = _need(chain, d, ext, fb, mfb, max(N, 0), max(chunk_samples, 0))
    return lib().rdyn_rollout_model_feedback(chain._h, C.byref(b) if batch else None, C.byref(d) if desc else None,
                                             C.cast(comps, C.c_void_p) if comps is not None else None, n_comps, _ref(ext), _ref(fb), _ref(mfb),
                                             chunk_samples, workspace, workspace_bytes)


def _refused(what=None):
    from rosdyn_amd._lib import lib
    msg = lib().rdyn_last_error()
    assert msg.startswith(WHO + b":"), msg
    if what is not None:
        assert what in msg, msg


def test_the_symbols_exist_with_the_documented_signatures():
    from rosdyn_amd import _lib
    flat = re.sub(r"\s+", " ", open(ROOT + "/include/rdyn.h").read())
    assert ("size_t rdyn_rollout_model_feedback_workspace_bytes(const rdyn_chain* chain, const rdyn_rollout_desc* desc, const rdyn_ext_wrenches* ext, "
            "const rdyn_feedback* fb, const rdyn_model_feedback* mfb, int64_t n_samples, int64_t chunk_samples);") in flat
    assert ("int rdyn_rollout_model_feedback(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_desc* desc, "
            "const rdyn_component* comps, int n_comps, const rdyn_ext_wrenches* ext, const rdyn_feedback* fb, const rdyn_model_feedback* mfb, "
            "int64_t chunk_samples, void* workspace, size_t workspace_bytes);") in flat
    assert flat.index("int rdyn_rollout_feedback(") < flat.index("typedef struct rdyn_model_feedback")   # declared after rdyn_rollout_feedback
    assert "typedef enum rdyn_feedback_law { RDYN_LAW_GRAVITY_COMPENSATION = 1, RDYN_LAW_COMPUTED_TORQUE = 2 } rdyn_feedback_law;" in flat
    l = _lib.lib()
    for name, nargs in (("rdyn_rollout_model_feedback", 11), ("rdyn_rollout_model_feedback_workspace_bytes", 7)):
        assert getattr(l, name) is not None and len(_lib.SYMBOLS[name][1]) == nargs
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct rdyn_model_feedback \{(.*?)\} rdyn_model_feedback;", flat).group(1))
    declared = [re.search(r"(\w+)$", decl.strip()).group(1) for decl in body.split(";") if decl.strip()]
    assert declared == [f[0] for f in _lib.ModelFeedback._fields_] == ["model", "law", "ddq_ref"]
    assert C.sizeof(_lib.ModelFeedback) == 24 and C.sizeof(_lib.Feedback) == 64   # rdyn_feedback keeps its size
    assert _lib.LAWS == {"gravity_compensation": GC_LAW, "computed_torque": CT_LAW}
    assert "Reverse mode is the follow-up" in flat


@pytest.mark.parametrize("name", SWEPT)
def test_no_samples_is_ok_and_every_refusal(name):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    model = chain.withParameters(chain.getNominalParameters() * 1.05)
    n, nj, N = chain.getActiveJointsNumber(), chain.getJointsNumber(), 7
    arr = _comps([(FRICTION1, 0), (SPRING, n - 1)])
    for m in (_mfb(model), _mfb(model, CT_LAW, FAKE), _mfb(model, GC_LAW), _mfb(chain)):
        for fb in (_fb(), _fb(dq_ref=None, kd=None, tau_limit=None), _fb(hold=0, gains_per_sample=1)):
            for x in (None, _ext(None), _ext(), _ext(link=nj)):
                for comps, k in ((None, 0), (arr, 2)):
                    assert _call(chain, 0, fb, m, x, comps, k) == RDYN_OK
                    assert _call(chain, 0, fb, m, x, comps, k, layout=1, integrator=EULER, q=None, dq=None, workspace=None, workspace_bytes=0) == RDYN_OK
    # fb is required once mfb is given
    for samples in (N, 0):
        assert _call(chain, samples, None, _mfb(model)) == RDYN_ERR_INVALID_ARGUMENT
        _refused(b"without the feedback")
    # the model, the law, the acceleration reference
    assert _call(chain, N, _fb(), _mfb(None)) == RDYN_ERR_INVALID_ARGUMENT
    _refused(b"null model")
    for law in (0, 3, -1, 1 << 20):
        assert _call(chain, N, _fb(), _mfb(model, law)) == RDYN_ERR_INVALID_ARGUMENT, law
        _refused(b"unknown law")
    assert _call(chain, N, _fb(), _mfb(model, GC_LAW, FAKE)) == RDYN_ERR_INVALID_ARGUMENT
    _refused(b"ddq_ref")
    # every argument error of rdyn_rollout_feedback
    for kw in ({"q_ref": None}, {"kp": None}):
        assert _call(chain, N, _fb(**kw), _mfb(model)) == RDYN_ERR_INVALID_ARGUMENT, kw
        _refused(b"q_ref")
    for stride in (-1, 1, n * N - 1):
        assert _call(chain, N, _fb(ref_step_stride=stride), _mfb(model)) == RDYN_ERR_INVALID_ARGUMENT, stride
        _refused(b"ref_step_stride")
    for kw in ({"hold": 2}, {"hold": -1}, {"gains_per_sample": 2}):
        assert _call(chain, N, _fb(**kw), _mfb(model)) == RDYN_ERR_INVALID_ARGUMENT, kw
        _refused(b"hold and gains_per_sample")
    for kw in ({"traj_every": 0, "traj_step_stride": n * N}, {"traj_every": 1, "traj_step_stride": n * N - 1}):
        assert _call(chain, N, _fb(tau_traj=FAKE), _mfb(model), **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
        _refused(b"trajectory")
    assert _call(chain, N, _fb(), _mfb(model), q_end=None, dq_end=None) == RDYN_ERR_INVALID_ARGUMENT
    _refused(b"every output is null")
    bad = _comps([(FRICTION1, n)])
    refusals = [
        {"desc": False}, {"tau": None}, {"n_steps": -1}, {"dt": 0.0}, {"dt": float("inf")}, {"dt": float("nan")}, {"integrator": 2}, {"integrator": -1},
        {"q_traj": FAKE, "traj_every": 0, "traj_step_stride": n * N}, {"chunk_samples": -1}, {"q": None}, {"dq": None}, {"batch": False}, {"layout": 5},
        {"comps": None, "n_comps": 1}, {"comps": arr, "n_comps": -1}, {"comps": bad, "n_comps": 1}, {"comps": _comps([(7, 0)]), "n_comps": 1},
        {"ext": _ext(link=-2)}, {"ext": _ext(link=nj + 1)}, {"ext": _ext(step_stride=-1)}, {"ext": _ext(link=nj, step_stride=6 * N - 1)},
    ]
    for x in (_ext(), None):
        for kw in refusals:
            kw = dict({"ext": x}, **kw)
            assert _call(chain, N, _fb(), _mfb(model), **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
            assert lib().rdyn_last_error()
        assert _call(chain, -1, _fb(), _mfb(model), x) == RDYN_ERR_INVALID_ARGUMENT


def test_a_model_of_another_shape_is_refused():
    """another number of chain joints, another joint type, another input selection, another input order"""
    from rosdyn_amd import Chain
    from rosdyn_amd.urdf_gen import generated_revolute_chain
    f, base, tool = FILES["ur10_like"]
    chain = Chain(os.path.join(FIXTURES, f), base, tool)
    N = 7
    shorter = Chain(os.path.join(FIXTURES, f), base, "wrist_3_link")
    if shorter.getJointsNumber() != chain.getJointsNumber():
        assert _call(chain, N, _fb(), _mfb(shorter)) == RDYN_ERR_INVALID_ARGUMENT
        _refused(b"chain joints")
    other = Chain(generated_revolute_chain(5, 1005), "l0", "l5")
    assert _call(chain, N, _fb(), _mfb(other)) == RDYN_ERR_INVALID_ARGUMENT
    _refused(b"chain joints")
    # the same joint count, another joint type: mixed_joints against a revolute chain of its length
    f2, base2, tool2 = FILES["mixed_joints"]
    mixed = Chain(os.path.join(FIXTURES, f2), base2, tool2)
    nj = mixed.getJointsNumber()
    rev = Chain(generated_revolute_chain(nj, 1000 + nj), "l0", "l%d" % nj)
    assert _call(mixed, N, _fb(), _mfb(rev)) == RDYN_ERR_INVALID_ARGUMENT
    _refused(b"type")
    # input joints: one left out; the same ones in another order
    names = chain.getActiveJointsName()
    fewer = chain.clone()
    assert fewer.setInputJointsName(names[:-1])
    assert _call(chain, N, _fb(), _mfb(fewer)) == RDYN_ERR_INVALID_ARGUMENT
    _refused(b"input joints")
    permuted = chain.clone()
    assert permuted.setInputJointsName([names[i] for i in (4, 0, 5, 2, 1, 3)])
    assert _call(chain, N, _fb(), _mfb(permuted)) == RDYN_ERR_INVALID_ARGUMENT
    _refused(b"input joints")
    assert _call(permuted, N, _fb(), _mfb(chain)) == RDYN_ERR_INVALID_ARGUMENT
    _refused(b"input joints")
    # ... and the model that matches passes these checks: what is refused next is the component list
    bad = _comps([(FRICTION1, chain.getActiveJointsNumber())])
    from rosdyn_amd._lib import lib
    assert _call(permuted, N, _fb(), _mfb(permuted.withParameters(permuted.getNominalParameters())), None, bad, 1) == RDYN_ERR_INVALID_ARGUMENT
    assert b"component" in lib().rdyn_last_error()


@pytest.mark.parametrize("name", ["rev14", "gen20_permuted"])
def test_the_chunked_route_is_unsupported_and_its_query_answers_zero(name):
    chain = _chain(name)
    model = chain.withParameters(chain.getNominalParameters())
    n = chain.getActiveJointsNumber()
    for law in (GC_LAW, CT_LAW):
        assert _call(chain, 7, _fb(), _mfb(model, law)) == RDYN_ERR_UNSUPPORTED
        _refused(b"chunked route")
        for chunk in CHUNKS:
            for integrator in INTEGRATOR_CODES:
                for N in SAMPLES:
                    assert _need(chain, _desc(n, N, integrator=integrator), None, _fb(), _mfb(model, law), N, chunk) == 0
    # the argument errors come first
    assert _call(chain, 7, _fb(), _mfb(model, 0)) == RDYN_ERR_INVALID_ARGUMENT


def test_a_long_chain_with_a_reduced_companion_is_served_without_wrenches_only():
    from rosdyn_amd import Chain
    chain = Chain(os.path.join(FIXTURES, "ur10_public_long.urdf"), "base_link", "tcp")
    model = chain.withParameters(chain.getNominalParameters() * 0.97)
    assert _call(chain, 0, _fb(), _mfb(model)) == RDYN_OK
    bad = _comps([(FRICTION1, chain.getActiveJointsNumber())])
    assert _call(chain, 7, _fb(), _mfb(model), None, bad, 1) == RDYN_ERR_INVALID_ARGUMENT   # past the routing: the component list is next
    assert _call(chain, 7, _fb(), _mfb(model), _ext(link=chain.getJointsNumber())) == RDYN_ERR_UNSUPPORTED
    _refused(b"chunked route")


@pytest.mark.parametrize("name", SWEPT + ["rev14"])
def test_the_workspace_query(name):
    """mfb == NULL: the query of rdyn_rollout_feedback; with mfb: 0"""
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    model = chain.withParameters(chain.getNominalParameters())
    n = chain.getActiveJointsNumber()
    for x in (None, _ext(None, link=2, step_stride=77), _ext(), _ext(link=1)):
        for chunk in CHUNKS:
            for integrator in INTEGRATOR_CODES:
                for N in SAMPLES:
                    d = _desc(n, N, integrator=integrator)
                    for fb in (None, _fb(), _fb(hold=0, gains_per_sample=1, tau_traj=FAKE)):
                        assert _need(chain, d, x, fb, None, N, chunk) == lib().rdyn_rollout_feedback_workspace_bytes(chain._h, C.byref(d), _ref(x), _ref(fb), N, chunk)
                    assert _need(chain, d, x, _fb(), _mfb(model), N, chunk) == 0
    # mfb == NULL is rdyn_rollout_feedback: its refusals under its own name
    assert _call(chain, 7, _fb(hold=2), None) == RDYN_ERR_INVALID_ARGUMENT
    assert lib().rdyn_last_error().startswith(b"rdyn_rollout_feedback:")


def test_the_python_surface():
    import rosdyn_amd
    from rosdyn_amd import Chain, Feedback, ModelFeedback
    p = inspect.signature(ModelFeedback.__init__).parameters
    assert list(p)[1:] == ["model", "law", "q_ref", "kp", "kd", "Dq_ref", "DDq_ref", "hold", "tau_limit", "command_trajectory"]
    assert p["kd"].default is None and p["Dq_ref"].default is None and p["DDq_ref"].default is None and p["hold"].default is True
    assert p["tau_limit"].default is None and p["command_trajectory"].default is False
    assert rosdyn_amd.ModelFeedback is ModelFeedback and issubclass(ModelFeedback, Feedback)
    with pytest.raises(ValueError, match="unknown law"):
        ModelFeedback(None, "pid", None, None)
    with pytest.raises(ValueError, match="DDq_ref"):
        ModelFeedback(None, "gravity_compensation", None, None, DDq_ref=0)
    # reverse mode raises a clear error
    fb = ModelFeedback(None, "computed_torque", None, None)
    chain = Chain(os.path.join(FIXTURES, "planar_2r.urdf"), "base", "l2")
    with pytest.raises(NotImplementedError, match="model-based law"):
        chain.rolloutAdjoint(None, None, None, 1e-3, None, None, feedback=fb)
    with pytest.raises(NotImplementedError, match="model-based law"):
        chain.rolloutParameterAdjoint(None, None, None, 1e-3, None, None, feedback=fb)
    from rosdyn_amd import autograd
    for call in (autograd.rollout, autograd.closed_loop_rollout):
        with pytest.raises(NotImplementedError, match="model-based law"):
            call(chain, None, None, None, 1e-3, feedback=fb)
