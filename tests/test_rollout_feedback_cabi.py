"""CPU tests (no GPU, but for the marked facade comparison): the symbols, argument checks and workspace queries of rdyn_rollout_feedback
(include/rdyn.h), the Python keyword, and the C++ facade's overloads through tests/cpp/rollout_feedback_facade.cpp.  Nothing unmarked
touches a device: every call either has no samples or fails its checks first."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import FIXTURES, ROOT
from _arrays import _value
from _cabi import (CHUNKED, CHUNKS, EULER, FAKE, INTEGRATOR_CODES, RDYN_ERR_INVALID_ARGUMENT, RDYN_OK, RK4, SAMPLES, SWEPT, _batch, _chain, _comps,
                   _ext, _query, _rollout_desc as _desc)
from _chains import FACADE_CHAINS
from _components import FRICTION1, SPRING

WHO = b"rdyn_rollout_feedback"


def _fb(**kw):
    from rosdyn_amd._lib import Feedback
    f = Feedback()
    f.q_ref, f.dq_ref, f.ref_step_stride, f.kp, f.kd, f.gains_per_sample, f.hold, f.tau_limit, f.tau_traj = FAKE, FAKE, 0, FAKE, FAKE, 0, 1, FAKE, None
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def _need(chain, d, ext, fb, N, chunk=0):
    from rosdyn_amd._lib import lib
    return lib().rdyn_rollout_feedback_workspace_bytes(chain._h, C.byref(d), C.byref(ext) if ext is not None else None,
                                                       C.byref(fb) if fb is not None else None, N, chunk)


def _call(chain, N, fb, ext=None, comps=None, n_comps=0, desc=True, chunk_samples=0, workspace=FAKE, workspace_bytes=None, q=FAKE, dq=FAKE,
          batch=True, layout=0, **kw):
    from rosdyn_amd._lib import lib
    b = _batch(N, q, dq, layout)
    d = _desc(chain.getActiveJointsNumber(), max(N, 0), **kw)
    if workspace_bytes is None:
        workspace_bytes = _need(chain, d, ext, fb, max(N, 0), max(chunk_samples, 0))
    return lib().rdyn_rollout_feedback(chain._h, C.byref(b) if batch else None, C.byref(d) if desc else None,
                                       C.cast(comps, C.c_void_p) if comps is not None else None, n_comps, C.byref(ext) if ext is not None else None,
                                       C.byref(fb) if fb is not None else None, chunk_samples, workspace, workspace_bytes)


def _refused(what=None):
    from rosdyn_amd._lib import lib
    msg = lib().rdyn_last_error()
    assert msg.startswith(WHO + b":"), msg
    if what is not None:
        assert what in msg, msg


def test_the_symbols_exist_with_the_documented_signatures():
    from rosdyn_amd import _lib
    flat = re.sub(r"\s+", " ", open(ROOT + "/include/rdyn.h").read())
    assert ("size_t rdyn_rollout_feedback_workspace_bytes(const rdyn_chain* chain, const rdyn_rollout_desc* desc, const rdyn_ext_wrenches* ext, "
            "const rdyn_feedback* fb, int64_t n_samples, int64_t chunk_samples);") in flat
    assert ("int rdyn_rollout_feedback(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_desc* desc, const rdyn_component* comps, "
            "int n_comps, const rdyn_ext_wrenches* ext, const rdyn_feedback* fb, int64_t chunk_samples, void* workspace, "
            "size_t workspace_bytes);") in flat
    l = _lib.lib()
    for name, nargs in (("rdyn_rollout_feedback", 10), ("rdyn_rollout_feedback_workspace_bytes", 6)):
        assert getattr(l, name) is not None and len(_lib.SYMBOLS[name][1]) == nargs
    # five pointers, an int64, two int32 sharing a word, a pointer, a pointer: the struct of include/rdyn.h field by field
    assert C.sizeof(_lib.Feedback) == 64
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct rdyn_feedback \{(.*?)\} rdyn_feedback;", flat).group(1))
    declared = [re.search(r"(\w+)$", decl.strip()).group(1) for decl in body.split(";") if decl.strip()]
    assert declared == [f[0] for f in _lib.Feedback._fields_]
    assert declared == ["q_ref", "dq_ref", "ref_step_stride", "kp", "kd", "gains_per_sample", "hold", "tau_limit", "tau_traj"]
    assert "rosdyn_amd.autograd does not serve the closed loop yet" in flat
    assert "fma(kd_j, Dq_ref[t]_j - Dq_j, fma(kp_j, q_ref[t]_j - q_j, tau_ff[t]_j))" in flat


@pytest.mark.parametrize("name", SWEPT + CHUNKED)
def test_no_samples_is_ok_and_every_refusal(name):
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n, nj, N = chain.getActiveJointsNumber(), chain.getJointsNumber(), 7
    arr = _comps([(FRICTION1, 0), (SPRING, n - 1)])
    for fb in (_fb(), _fb(dq_ref=None, kd=None, tau_limit=None), _fb(hold=0, gains_per_sample=1, ref_step_stride=0), None):
        for x in (None, _ext(None), _ext(), _ext(link=nj)):
            for comps, k in ((None, 0), (arr, 2)):
                assert _call(chain, 0, fb, x, comps, k) == RDYN_OK
                assert _call(chain, 0, fb, x, comps, k, layout=1, integrator=EULER, q=None, dq=None, workspace=None, workspace_bytes=0) == RDYN_OK
    # the references and the gains
    for kw in ({"q_ref": None}, {"kp": None}):
        for samples in (N, 0):
            assert _call(chain, samples, _fb(**kw)) == RDYN_ERR_INVALID_ARGUMENT, kw
            _refused(b"q_ref")
    # the step stride of the references: negative; not zero and below one step's record
    for stride in (-1, 1, n * N - 1, -n * N):
        assert _call(chain, N, _fb(ref_step_stride=stride)) == RDYN_ERR_INVALID_ARGUMENT, stride
        _refused(b"ref_step_stride")
    # hold and gains_per_sample are flags
    for kw in ({"hold": 2}, {"hold": -1}, {"gains_per_sample": 2}, {"gains_per_sample": -1}, {"hold": 1 << 20}):
        assert _call(chain, N, _fb(**kw)) == RDYN_ERR_INVALID_ARGUMENT, kw
        _refused(b"hold and gains_per_sample")
    # the command record needs what the state records need, and counts as an output
    for kw in ({"traj_every": 0, "traj_step_stride": n * N}, {"traj_every": 1, "traj_step_stride": n * N - 1}, {"traj_every": -1, "traj_step_stride": n * N}):
        assert _call(chain, N, _fb(tau_traj=FAKE), **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
        _refused(b"trajectory")
    assert _call(chain, N, _fb(), q_end=None, dq_end=None) == RDYN_ERR_INVALID_ARGUMENT
    _refused(b"every output is null")
    # ... the smallest valid values pass the feedback checks: what is refused next is the component list
    bad = _comps([(FRICTION1, n)])
    for fb, kw in ((_fb(ref_step_stride=n * N), {}), (_fb(tau_traj=FAKE), {"q_end": None, "dq_end": None, "traj_every": 1, "traj_step_stride": n * N}),
                   (_fb(hold=0, gains_per_sample=1), {})):
        assert _call(chain, N, fb, None, bad, 1, **kw) == RDYN_ERR_INVALID_ARGUMENT
        assert b"component" in lib().rdyn_last_error()   # (the shared component check's own text)
    # every argument error of rdyn_rollout_ext, with and without wrenches, with and without the feedback
    refusals = [
        {"desc": False}, {"tau": None}, {"q_end": None, "dq_end": None}, {"n_steps": -1},
        {"dt": 0.0}, {"dt": float("inf")}, {"dt": float("nan")}, {"integrator": 2}, {"integrator": -1},
        {"q_traj": FAKE, "traj_every": 0, "traj_step_stride": n * N}, {"q_traj": FAKE, "traj_every": 1, "traj_step_stride": n * N - 1},
        {"chunk_samples": -1}, {"q": None}, {"dq": None}, {"batch": False}, {"layout": 5},
        {"comps": None, "n_comps": 1}, {"comps": arr, "n_comps": -1}, {"comps": bad, "n_comps": 1}, {"comps": _comps([(7, 0)]), "n_comps": 1},
        {"ext": _ext(link=-2)}, {"ext": _ext(link=nj + 1)}, {"ext": _ext(step_stride=-1)}, {"ext": _ext(link=nj, step_stride=6 * N - 1)},
    ]
    for fb in (_fb(), None):
        for x in (_ext(), None):
            for kw in refusals:
                kw = dict({"ext": x}, **kw)
                assert _call(chain, N, fb, **kw) == RDYN_ERR_INVALID_ARGUMENT, kw
                assert lib().rdyn_last_error()
            assert _call(chain, -1, fb, x) == RDYN_ERR_INVALID_ARGUMENT
    assert lib().rdyn_rollout_feedback(None, None, None, None, 0, None, None, 0, FAKE, 1 << 30) == RDYN_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", SWEPT + CHUNKED)
def test_the_workspace_query(name):
    """fb == NULL: the query of rdyn_rollout_ext.  With the feedback: 0 where that query answers 0 (chains swept in registers), otherwise
    that figure plus one state array, align256(n N 8) -- the formula of include/rdyn.h."""
    from rosdyn_amd._lib import lib
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    align256 = lambda b: (b + 255) // 256 * 256
    for x in (None, _ext(None, link=2, step_stride=77), _ext(), _ext(link=1)):
        px = C.byref(x) if x is not None else None
        for chunk in CHUNKS:
            for integrator in INTEGRATOR_CODES:
                for N in SAMPLES:
                    d = _desc(n, N, integrator=integrator)
                    base = lib().rdyn_rollout_ext_workspace_bytes(chain._h, C.byref(d), px, N, chunk)
                    assert _need(chain, d, x, None, N, chunk) == base
                    for fb in (_fb(), _fb(hold=0, gains_per_sample=1, tau_traj=FAKE)):
                        got = _need(chain, d, x, fb, N, chunk)
                        assert got == (base + align256(n * N * 8) if base else 0), (chunk, integrator, N)
                        assert (got == 0) == (name in SWEPT)
    if name in CHUNKED:   # an undersized workspace is refused: the extra array counts
        d = _desc(n, 7)
        need = _need(chain, d, None, _fb(), 7, 1000)
        assert need == _query(chain, d, 7, 1000) + align256(n * 7 * 8)
        assert _call(chain, 7, _fb(), chunk_samples=1000, workspace_bytes=need - 1) == RDYN_ERR_INVALID_ARGUMENT
        _refused(b"workspace too small")
        assert _call(chain, 7, _fb(), chunk_samples=1000, workspace_bytes=_query(chain, d, 7, 1000)) == RDYN_ERR_INVALID_ARGUMENT
        assert _call(chain, 7, _fb(), chunk_samples=1000, workspace=None, workspace_bytes=need) == RDYN_ERR_INVALID_ARGUMENT


def test_a_long_chain_with_a_reduced_companion_needs_the_array_with_wrenches_only():
    from rosdyn_amd import Chain
    chain = Chain(os.path.join(FIXTURES, "ur10_public_long.urdf"), "base_link", "tcp")
    n = chain.getActiveJointsNumber()
    d = _desc(n, 7)
    assert _need(chain, d, None, _fb(), 7, 1000) == 0
    x = _ext(link=chain.getJointsNumber())
    from rosdyn_amd._lib import lib
    base = lib().rdyn_rollout_ext_workspace_bytes(chain._h, C.byref(d), C.byref(x), 7, 1000)
    assert base > 0 and _need(chain, d, x, _fb(), 7, 1000) == base + (n * 7 * 8 + 255) // 256 * 256


def test_the_python_surface():
    import rosdyn_amd
    from rosdyn_amd import Chain, Feedback
    assert inspect.signature(Chain.rollout).parameters["feedback"].default is None
    p = inspect.signature(Feedback.__init__).parameters
    assert list(p)[1:] == ["q_ref", "kp", "kd", "Dq_ref", "hold", "tau_limit", "command_trajectory"]
    assert p["kd"].default is None and p["Dq_ref"].default is None and p["hold"].default is True and p["tau_limit"].default is None
    assert p["command_trajectory"].default is False and rosdyn_amd.Feedback is Feedback


# ---- the C++ facade
def _build(tmp_path):
    exe = tmp_path / "rollout_feedback_facade"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "tests", "mock_include"), "-I" + os.path.join(ROOT, "rosdyn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "rollout_feedback_facade.cpp"), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "rosdyn_amd"), "-lrdyn_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "rosdyn_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def test_the_facade_caller_builds_pedantic_against_the_stand_in_eigen_headers(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("urdf,base,tool", FACADE_CHAINS)
def test_the_facade_gives_the_python_binding_own_bits(tmp_path, urdf, base, tool):
    torch = pytest.importorskip("torch")
    from rosdyn_amd import Chain, Feedback
    exe = _build(tmp_path)
    r = subprocess.run([exe, os.path.join(FIXTURES, urdf), base, tool], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout + r.stderr
    got = {ln.split()[0]: np.array([float(x) for x in ln.split()[1:]]) for ln in r.stdout.splitlines() if " " in ln}
    chain = Chain(os.path.join(FIXTURES, urdf), base, tool, (0.0, 0.0, -9.806))
    n, N, T = chain.getActiveJointsNumber(), 5, 3
    grid = lambda k, m=n: np.array([[_value(s, i, k) for i in range(m)] for s in range(N)])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    q, dq = dev(grid(0)), dev(grid(1))
    tau = dev(np.stack([0.5 * grid(2 + t) for t in range(T)]))
    q_ref, dq_ref = dev(np.stack([grid(20 + t) for t in range(T)])), dev(np.stack([grid(30 + t) for t in range(T)]))
    kp, kd, lim = dev(4.0 + np.arange(n)), dev(0.5 + 0.25 * np.arange(n)), dev(np.full(n, 2.0))
    w_tool = dev(0.5 * grid(12, 6))
    fb = Feedback(q_ref, kp, kd, dq_ref, hold=True, tau_limit=lim, command_trajectory=True)
    q1, dq1, st, _, _, ut = chain.rollout(q, dq, tau, 1e-3, integrator="rk4", trajectory_every=1, feedback=fb)
    assert bool((st == 1).all())
    assert np.array_equal(got["q_end"], q1.cpu().numpy().ravel()) and np.array_equal(got["dq_end"], dq1.cpu().numpy().ravel())
    assert np.array_equal(got["u_last"], ut[T - 1].cpu().numpy().ravel())
    fb = Feedback(q_ref, kp, kd, dq_ref, hold=False, tau_limit=lim)
    q2, dq2, st = chain.rollout(q, dq, tau, 1e-3, integrator="rk4", feedback=fb, ext_wrenches=w_tool, ext_link=chain.getLinksName()[-1])
    assert bool((st == 1).all())
    assert np.array_equal(got["q_end_tool"], q2.cpu().numpy().ravel()) and np.array_equal(got["dq_end_tool"], dq2.cpu().numpy().ravel())
    assert not np.array_equal(got["q_end_tool"], got["q_end"])
