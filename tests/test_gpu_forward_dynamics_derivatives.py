"""GPU tests of rdyn_forward_dynamics_derivatives / Chain.getJointAccelerationDerivatives: with ddq = FD_c(q, dq, tau)
    dddq_dq = -M^-1 (dtau_dq + diag d tau_c / d q),  dddq_dv = -M^-1 (dtau_dv + diag d tau_c / d dq),  minv = M^-1,
dtau_dq, dtau_dv the derivatives of the joint torque at that very ddq.

Oracle, residual form (every sample, none excused).  With ddq the library's own output, D_ref is the exact spectral / central-difference
derivative of the oracle torque at that ddq (test_gpu_torque_derivatives.py; its 8-against-16-point gap is asserted <= 1e-12) and
    |M_ref X + D_ref|_inf <= 1e-11 (|M_ref|_inf |X|_inf + |D_ref|_inf + |tau_ref|_inf)     X = dddq_dq, dddq_dv
    |M_ref minv - 1|_inf  <= 1e-11 (|M_ref|_inf |minv|_inf + 1)
(|M_ref|_inf the largest absolute row sum).  1e-11 is the project's parity figure for M and D; a backward-stable Cholesky solve adds
c n eps ~ 1e-14 in the same units.

Components: the same residuals with D_ref + diag(slopes), the slopes from the closed form written here (_slopes), which a five-point
stencil (exact for the cubic pieces of the friction polynomials; h = 2^-10; rounding 1.5 eps / h ~ 3.4e-13 of the differenced torque) pins
to oracle/components_oracle.c on every entry at least 2^-8 away from the four kinks +-min_velocity, +-max_velocity: bound
1e-11 (|slope| + max|tau_c| / h); at most 5 % of the entries may be left out (expected: 4 kinks x 2 x 2^-8 / 2 = 1.6 %).

Directional consistency (not a parity bound): dddq_dq e + dddq_dv f + minv g against the central difference of getJointAcceleration along
(e, f, g), entries in +-1, h = 2^-7 and 2^-8, scale = max|terms| + |ddq|_inf.  FD is smooth, so the error of the central difference is
h^2 / 6 |FD'''| + O(h^4).  Measured on the CPU ORACLE alone with this test's own inputs (_directional_inputs, N = 1000: exact -M_ref^-1 D_ref
and M_ref^-1 against the central difference of the oracle's own forward dynamics):
    chain          err(2^-7) / scale, worst    err(2^-7) / err(2^-8)    samples >= 1e-9 scale
    ur10_public    3.82e-5                     [3.9992, 4.0023]         1000 of 1000
    mixed_joints   1.02e-4                     [3.9946, 4.0030]          998 of 1000
    panda_like     2.26e-3                     [3.9886, 4.0049]         1000 of 1000
    rev14          1.82e-4                     [3.9989, 4.0010]         1000 of 1000
    gen20          6.87e-4                     [3.9948, 4.0049]         1000 of 1000
Asserted: err(2^-7) <= 20 x the measured worst of the chain (DIRECTIONAL_WORST; the margin test_gpu_torque_derivatives.py takes for the
same reason: a wrong term shows at order 1), and the ratio in [3.5, 4.5] on the samples with err(2^-7) >= 1e-9 scale, which must be at
least half of the batch.

minv is symmetric BITWISE: a unit column is solved at and below its diagonal and mirrored."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import FIXTURES, ROOT
from _arrays import DERIVATIVE_NAMES as NAMES, _derivatives_call as _call, _dev, _host, _inputs
from _chains import GRAV, _chain, _pair
from _components import MAX_VELOCITY, MIN_VELOCITY, _pin_the_closed_form_to_the_oracle, _set, _slopes, _specs
from _references import _derivative_residual_ratios as _residual_ratios, _input_types
from rosdyn_amd.urdf_gen import generated_revolute_chain

pytestmark = pytest.mark.gpu
# worst err(2^-7) / scale of the oracle's own directional check, this module's inputs (the docstring's table)
DIRECTIONAL_WORST = {"ur10_public": 3.82e-5, "mixed_joints": 1.02e-4, "panda_like": 2.26e-3, "rev14": 1.82e-4, "gen20": 6.87e-4}


ORACLE_CHAINS = ["planar_2r", "rev1", "mixed_joints", "ur10_public", "panda_like", "ur10_public_long", "rev8", "rev10", "rev14",
                 "gen20_permuted", "rev32"]
CASES = [(name, N) for name in ORACLE_CHAINS for N in (1, 63, 64, 65, 200)] + [("ur10_public", 4096), ("panda_like", 4096)]


# ---- 1. the oracle, residual form
@pytest.mark.parametrize("layout", ["sample", "element"])
@pytest.mark.parametrize("name,N", CASES)
def test_against_the_oracle_in_residual_form(name, N, layout):
    torch = pytest.importorskip("torch")
    chain, ref = _pair(name)
    n = ref.n
    q, dq, tau = _inputs(n, N)
    ddq, st, Xq, Xv, Minv = _call(torch, chain, q, dq, tau, layout)
    assert st.shape == (N,) and (st == 1).all(), np.unique(st)
    assert ddq.shape == (N, n) and all(X.shape == (N, n, n) and np.isfinite(X).all() for X in (Xq, Xv, Minv))
    plain, st2 = chain.getJointAcceleration(_dev(torch, q, layout), _dev(torch, dq, layout), _dev(torch, tau, layout), layout=layout)
    assert np.array_equal(_host(plain, layout), ddq) and (st2.cpu().numpy() == 1).all()
    R = min(N, 256)
    worst = _residual_ratios(ref, _input_types(chain), q[:R], dq[:R], ddq[:R], Xq[:R], Xv[:R], Minv[:R])
    print("%s %s N=%d: worst residual ratio dddq_dq %.3g dddq_dv %.3g minv %.3g (bound 1e-11)"
          % (name, layout, N, worst["dddq_dq"], worst["dddq_dv"], worst["minv"]))
    for what, r in worst.items():
        assert r <= 1e-11, (what, r)


# ---- 2. components


@pytest.mark.parametrize("name", ["ur10_public", "mixed_joints", "rev14"])
def test_components_put_their_slopes_on_the_diagonals(name):
    torch = pytest.importorskip("torch")
    chain, ref = _pair(name)
    n, N = ref.n, 200
    specs = _specs(n)
    cs = _set(specs, n)
    q, dq, tau = _inputs(n, N, seed=4100)
    band = (np.abs(dq) < MIN_VELOCITY).mean()
    sat = (np.abs(dq) > MAX_VELOCITY).mean()
    assert 0.2 < band < 0.4 and 0.1 < sat < 0.3, (band, sat)
    _pin_the_closed_form_to_the_oracle(specs, n, q, dq)
    for layout in ("sample", "element"):
        ddq, st, Xq, Xv, Minv = _call(torch, chain, q, dq, tau, layout, components=cs)
        assert (st == 1).all()
        want, _ = chain.getJointAcceleration(_dev(torch, q, layout), _dev(torch, dq, layout), _dev(torch, tau, layout), layout=layout, components=cs)
        assert np.array_equal(_host(want, layout), ddq)
        worst = _residual_ratios(ref, _input_types(chain), q, dq, ddq, Xq, Xv, Minv, slopes=_slopes(specs, q, dq))
        print("%s %s with components: worst residual ratio dddq_dq %.3g dddq_dv %.3g minv %.3g (bound 1e-11)"
              % (name, layout, worst["dddq_dq"], worst["dddq_dv"], worst["minv"]))
        for what, r in worst.items():
            assert r <= 1e-11, (what, r)
        # the slopes matter at this bound: without them the residual is far off
        bare = _residual_ratios(ref, _input_types(chain), q, dq, ddq, Xq, Xv, Minv)
        assert bare["dddq_dq"] > 1e-6 and bare["dddq_dv"] > 1e-6, bare
        # an empty list is the plain call, bitwise
        a = _call(torch, chain, q, dq, tau, layout, components=_set([], n))
        b = _call(torch, chain, q, dq, tau, layout)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


# ---- 3. directional consistency
def _directional_inputs(n, N=1000):
    from rosdyn_amd.samples import uniform_pm1
    q, dq, tau = _inputs(n, N, seed=5100)
    e, f, g = (uniform_pm1(5110 + i, (N, n)) for i in range(3))
    return q, dq, tau, e, f, g


@pytest.mark.parametrize("name", sorted(DIRECTIONAL_WORST))
def test_directional_consistency_with_central_differences_of_the_forward_dynamics(name):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 1000
    q, dq, tau, e, f, g = (torch.from_numpy(x).cuda() for x in _directional_inputs(n, N))
    ddq, st, Xq, Xv, Minv = chain.getJointAccelerationDerivatives(q, dq, tau)   # [s, k, i]
    assert bool((st == 1).all())
    terms = [torch.einsum("ski,sk->si", X, d) for X, d in ((Xq, e), (Xv, f), (Minv, g))]
    lin = terms[0] + terms[1] + terms[2]
    scale = torch.stack([t.abs().amax(dim=1) for t in terms]).amax(dim=0) + ddq.abs().amax(dim=1)
    errs = []
    for h in (2.0 ** -7, 2.0 ** -8):
        up, _ = chain.getJointAcceleration(q + h * e, dq + h * f, tau + h * g)
        dn, _ = chain.getJointAcceleration(q - h * e, dq - h * f, tau - h * g)
        errs.append(((up - dn) / (2.0 * h) - lin).abs().amax(dim=1) / scale)
    sel = errs[0] >= 1e-9
    ratio = errs[0][sel] / errs[1][sel]
    bound = 20.0 * DIRECTIONAL_WORST[name]
    print("%s N=%d: directional err(2^-7) max %.3g (bound %.3g), err ratio %.4g .. %.4g over %d samples (bounds 3.5, 4.5)"
          % (name, N, float(errs[0].max()), bound, float(ratio.min()), float(ratio.max()), int(sel.sum())))
    assert float(errs[0].max()) <= bound
    assert int(sel.sum()) >= N // 2 and float(ratio.min()) >= 3.5 and float(ratio.max()) <= 4.5


# ---- 4. identities
@pytest.mark.parametrize("name", ["panda_like", "rev10", "gen20_permuted"])
def test_symmetric_inverse_layouts_and_subsets_agree_bitwise(name):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 4096
    q, dq, tau = _inputs(n, N, seed=4400)
    full = _call(torch, chain, q, dq, tau, "sample")
    assert (full[1] == 1).all()
    assert np.array_equal(full[4], np.swapaxes(full[4], 1, 2))   # minv: the same bits in both triangles
    el = _call(torch, chain, q, dq, tau, "element")
    for x, y in zip(full, el):
        assert np.array_equal(x, y)
    for layout, whole in (("sample", full), ("element", el)):
        for mask in range(1, 7):
            want = tuple(k for b, k in enumerate(NAMES) if mask >> b & 1)
            part = _call(torch, chain, q, dq, tau, layout, want=want)
            assert np.array_equal(part[0], whole[0]) and np.array_equal(part[1], whole[1])
            for k, t in zip(want, part[2:]):
                assert np.array_equal(t, whole[2 + NAMES.index(k)]), (layout, want, k)


# ---- 5. not positive definite
@pytest.mark.parametrize("layout", ["sample", "element"])
def test_inertia_that_is_not_positive_definite_reports_minus_one_and_nan(layout):
    """ur10_public with the fixed joint of tool0 among the input joints: its row and column of M are zero."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd import Chain
    chain = Chain(os.path.join(FIXTURES, "ur10_public.urdf"), "base_link", "tool0", GRAV)
    moving = ["shoulder_pan_joint", "shoulder_lift_joint", "elbow_joint", "wrist_1_joint", "wrist_2_joint", "wrist_3_joint"]
    assert chain.setInputJointsName(moving[:3] + ["flange-tool0"] + moving[3:])
    n, N = 7, 200
    q, dq, tau = _inputs(n, N, seed=33)
    ddq, st, Xq, Xv, Minv = _call(torch, chain, q, dq, tau, layout)
    assert (st == -1).all() and np.isnan(ddq).all()
    assert np.isnan(Xq).all() and np.isnan(Xv).all() and np.isnan(Minv).all()
    # a valid chain in the same process afterwards still answers correctly
    good, ref = _pair("ur10_public")
    q, dq, tau = _inputs(ref.n, N, seed=34)
    ddq, st, Xq, Xv, Minv = _call(torch, good, q, dq, tau, layout)
    assert (st == 1).all()
    worst = _residual_ratios(ref, _input_types(good), q, dq, ddq, Xq, Xv, Minv)
    for what, r in worst.items():
        assert r <= 1e-11, (what, r)


# ---- 6. plumbing
def _raw(chain, N, layout, tq, tdq, tau_ptr, ddq_ptr, mats, status_ptr, chunk=0, ws=None, stream=None):
    import torch
    from rosdyn_amd._lib import Batch, check, lib
    b = Batch()
    b.n_samples = N
    b.q, b.dq, b.ddq = tq.data_ptr(), tdq.data_ptr(), None
    b.layout = 1 if layout == "element" else 0
    b.device = -1
    b.stream = (stream or torch.cuda.current_stream()).cuda_stream
    check(lib().rdyn_forward_dynamics_derivatives(chain._h, C.byref(b), None, 0, tau_ptr, ddq_ptr, mats[0], mats[1], mats[2], status_ptr, chunk,
                                                  ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0))


def _workspace(torch, chain, chunk=0):
    from rosdyn_amd._lib import lib
    nbytes = lib().rdyn_forward_dynamics_derivatives_workspace_bytes(chain._h, chunk)
    return torch.empty((nbytes,), dtype=torch.uint8, device="cuda") if nbytes else None


@pytest.mark.parametrize("name", ["ur10_like", "rev10", "rev14"])
def test_plumbing_alias_null_status_unaligned_outputs_and_guard_bands(name):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 1000
    nn = n * n
    q, dq, tau = _inputs(n, N, seed=11)
    ws = _workspace(torch, chain)
    for layout in ("sample", "element"):
        tq, tdq, ttau = _dev(torch, q, layout), _dev(torch, dq, layout), _dev(torch, tau, layout)
        full = chain.getJointAccelerationDerivatives(tq, tdq, ttau, layout=layout)
        assert bool((full[1] == 1).all())
        assert np.array_equal(_host(ttau, layout), tau)   # the torques are left alone when ddq does not alias them
        # every matrix 8 bytes off a 128-byte line inside poisoned guard bands; ddq aliasing tau; status NULL
        G = 16
        bufs = [torch.full((G + 1 + N * nn + G,), 12345.5, dtype=torch.float64, device="cuda") for _ in range(3)]
        outs = [b[G + 1:G + 1 + N * nn] for b in bufs]
        assert all(o.data_ptr() % 128 == 8 for o in outs)
        buf = _dev(torch, tau, layout)
        _raw(chain, N, layout, tq, tdq, buf.data_ptr(), buf.data_ptr(), [o.data_ptr() for o in outs], None, ws=ws)
        torch.cuda.synchronize()
        assert torch.equal(buf, full[0])
        for o, b, t in zip(outs, bufs, full[2:]):
            assert torch.equal(o.view(t.shape), t), layout
            assert (b[:G + 1] == 12345.5).all() and (b[G + 1 + N * nn:] == 12345.5).all()
        # guard bands around ddq and status
        big = torch.full((G + 1 + N * n + G,), 12345.5, dtype=torch.float64, device="cuda")
        sbig = torch.full((G + N + G,), 777, dtype=torch.int32, device="cuda")
        out = big[G + 1:G + 1 + N * n]
        mats = [torch.empty_like(t) for t in full[2:]]
        _raw(chain, N, layout, tq, tdq, ttau.data_ptr(), out.data_ptr(), [m.data_ptr() for m in mats], sbig[G:].data_ptr(), ws=ws)
        torch.cuda.synchronize()
        assert torch.equal(out.view(full[0].shape), full[0])
        assert (big[:G + 1] == 12345.5).all() and (big[G + 1 + N * n:] == 12345.5).all()
        assert (sbig[:G] == 777).all() and (sbig[G + N:] == 777).all() and (sbig[G:G + N] == 1).all()
        for m, t in zip(mats, full[2:]):
            assert torch.equal(m, t)
        assert np.array_equal(_host(ttau, layout), tau)


# ---- 7. chunk size
def test_chunk_size_does_not_change_the_result():
    torch = pytest.importorskip("torch")
    chain = _chain("rev20")
    n, N = 20, 40000
    q, dq, tau = _inputs(n, N, seed=21)
    a = _call(torch, chain, q, dq, tau, "sample", chunk_samples=16384)
    b = _call(torch, chain, q, dq, tau, "sample", chunk_samples=(N + 2) // 3)
    c = _call(torch, chain, q, dq, tau, "element", chunk_samples=1000)
    assert (a[1] == 1).all()
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)


# ---- 8. graph
@pytest.mark.parametrize("name", ["ur10_like", "rev14"])
def test_replays_from_a_captured_graph(name):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 20000
    q, dq, tau = (torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(3))
    ddq = torch.empty_like(q)
    st = torch.empty((N,), dtype=torch.int32, device="cuda")
    outs = [torch.empty((N, n, n), dtype=torch.float64, device="cuda") for _ in range(3)]
    ws = _workspace(torch, chain, 8192)
    ptrs = [o.data_ptr() for o in outs]
    _raw(chain, N, "sample", q, dq, tau.data_ptr(), ddq.data_ptr(), ptrs, st.data_ptr(), chunk=8192, ws=ws)   # first use outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            _raw(chain, N, "sample", q, dq, tau.data_ptr(), ddq.data_ptr(), ptrs, st.data_ptr(), chunk=8192, ws=ws, stream=s)
    for k in range(3):
        q.uniform_(-1, 1)
        dq.uniform_(-1, 1)
        tau.uniform_(-50, 50)
        ddq.zero_()
        st.zero_()
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        again = chain.getJointAccelerationDerivatives(q, dq, tau, chunk_samples=8192)
        assert torch.equal(ddq, again[0]) and torch.equal(st, again[1]) and bool((st == 1).all())
        for o, t in zip(outs, again[2:]):
            assert torch.equal(o, t)


# ---- 9. facade
def test_facade_batch_method_and_single_sample_getter(tmp_path):
    """tests/cpp/forward_dynamics_derivatives_facade.cpp: getJointAccelerationDerivativesBatch and getJointAccelerationDerivatives of the
    C++ facade (6 joints in registers, 14 input joints through the chunked route, components)."""
    exe = tmp_path / "fdd_facade"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "rosdyn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "forward_dynamics_derivatives_facade.cpp"),
                           "-o", str(exe), "-L" + os.path.join(ROOT, "rosdyn_amd"), "-lrdyn_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "rosdyn_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    long_urdf = tmp_path / "rev14.urdf"
    long_urdf.write_text(generated_revolute_chain(14, 1014))
    r = subprocess.run([str(exe), os.path.join(FIXTURES, "ur10_like.urdf"), os.path.join(FIXTURES, "ur10_public.urdf"), str(long_urdf)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
