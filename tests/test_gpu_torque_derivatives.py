"""GPU tests of rdyn_joint_torque_derivatives / Chain.getJointTorqueDerivatives: dtau/dq, dtau/dDq and M = dtau/dDDq of the function
rdyn_joint_torque evaluates for the chain as configured.

The reference derivative is EXACT, built from OracleChain.joint_torque alone: as a function of one revolute q_k every tau_i is a
trigonometric polynomial of degree <= 2 (harmonics >= 3 at <= 2e-14 against amplitudes up to 1e2, checked with oracle/np_restatement.py),
as a function of a prismatic q_k and of any Dq_k a polynomial of degree <= 2.  So
  dtau/dq_k, revolute    spectral differentiation over 8 equispaced samples q_k + 2 pi m / 8 (exact through degree 3)
  dtau/dq_k, prismatic   one central difference with h = 1
  dtau/dDq_k             one central difference with h = 1
  M                      OracleChain.joint_inertia
Bound, every sample and every entry, no sample excused:  |D - D_ref| <= 1e-11 (max|D_ref| + |tau_ref|_inf) over that sample -- 1e-11 is the
project's parity figure, the tau term covers the rounding of the differenced torques.  The construction itself is asserted first: the
spectral reference on 8 and on 16 points agree to 1e-12 in the same units.
Exact identities between library calls: 1e-11 relative to the per-sample max magnitude of the terms.
Directional check (a consistency check, not a parity bound): dtau_dq e + dtau_dv f + M g against the central difference of
rdyn_joint_torque along (e, f, g), |e|, |f|, |g| <= 1 per entry, steps h = 2^-7 and 2^-8.  tau is smooth, so the error of the central
difference is h^2 / 6 |tau'''| + O(h^4) with a rounding floor eps |tau| / h ~ 3e-14 |tau|: measured on the ORACLE (its exact spectral
derivative against its own central difference; ur10_public, mixed_joints, panda_like, rev14, gen20, 256 samples each) err(2^-7) <= 1.8e-4
scale (gen20; 2.8e-5 at 6 and 7 joints), scale = max|terms| + |tau|_inf, smallest 2e-8, and err(2^-7) / err(2^-8) in [3.9995, 4.0001].  Asserted:
err(2^-7) <= 4e-3 scale (twenty times the measured worst, for batches a thousand times larger: a wrong term shows at order 1), and the
ratio in [3.5, 4.5] on the samples with err(2^-7) >= 1e-9 scale (at least half of the batch)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import FIXTURES, ROOT
from _arrays import _dev, _inf, _mat
from _chains import CHAINS, _chain, _pair, _spec
from _references import _input_types, _reference
from rosdyn_amd.urdf_gen import generated_revolute_chain

pytestmark = pytest.mark.gpu


def _inputs(n, N, seed=77):
    from rosdyn_amd.samples import uniform_pm1
    return uniform_pm1(seed, (N, n)), uniform_pm1(seed + 1, (N, n)), 3.0 * uniform_pm1(seed + 2, (N, n))


def _derivs(torch, chain, q, dq, ddq, layout, want=("dq", "dv", "M")):
    out = chain.getJointTorqueDerivatives(_dev(torch, q, layout), _dev(torch, dq, layout), _dev(torch, ddq, layout), layout=layout, want=want)
    return [_mat(t, layout) for t in out]


_REF = {}


def _cached_reference(name, N_ref, ref, types, q, dq, ddq):
    key = (name, N_ref)
    if key not in _REF:
        _REF[key] = _reference(ref, types, q[:N_ref], dq[:N_ref], ddq[:N_ref]) + (ref.joint_inertia(q[:N_ref]),)
    return _REF[key]


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("layout", ["sample", "element"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 200, 4096])
def test_against_the_exact_oracle_derivative(name, layout, N):
    torch = pytest.importorskip("torch")
    chain, ref = _pair(name)
    n = ref.n
    q, dq, ddq = _inputs(n, N)
    Dq, Dv, M = _derivs(torch, chain, q, dq, ddq, layout)
    assert Dq.shape == (N, n, n) and Dv.shape == (N, n, n) and M.shape == (N, n, n)
    assert np.isfinite(Dq).all() and np.isfinite(Dv).all() and np.isfinite(M).all()
    # chains over 10 input joints: the oracle comparison on the first 256 samples (the rest: the identity tests, at full batch)
    N_ref = min(N, 256) if n > 10 else N
    Dq_ref, Dv_ref, tau_ref, gap, M_ref = _cached_reference(name, N_ref, ref, _input_types(chain), q, dq, ddq)
    scale = np.maximum(_inf(Dq_ref), _inf(Dv_ref)) + _inf(tau_ref)
    assert (gap <= 1e-12 * scale).all(), ("spectral reference, 8 against 16 points", float((gap / scale).max()))
    worst = {}
    for what, got, want, sc in (("dtau_dq", Dq, Dq_ref, _inf(Dq_ref) + _inf(tau_ref)), ("dtau_dv", Dv, Dv_ref, _inf(Dv_ref) + _inf(tau_ref)),
                                ("M", M, M_ref, _inf(M_ref) + _inf(tau_ref))):
        ratio = _inf(got[:N_ref] - want) / sc
        worst[what] = float(ratio.max())
    print("%s %s N=%d: worst ratio dtau_dq %.3g dtau_dv %.3g M %.3g (bound 1e-11), construction gap %.3g (bound 1e-12)"
          % (name, layout, N, worst["dtau_dq"], worst["dtau_dv"], worst["M"], float((gap / scale).max())))
    for what, r in worst.items():
        assert r <= 1e-11, (what, r)


def _identity_sizes(name):
    return 1000000 if name in ("ur10_like", "panda_like") else 200000


def _rel(err, *terms):
    scale = np.maximum.reduce([_inf(t) for t in terms])
    return float((_inf(err) / np.maximum(scale, np.finfo(np.float64).tiny)).max())


@pytest.mark.parametrize("name", ["ur10_like", "panda_like", "rev14", "rev20"])
def test_identities_between_library_calls_at_full_size(name):
    """6 and 7 joints at 1e6 samples, 14 and 20 at 2e5; device arithmetic throughout (torch), bounds 1e-11 relative to the per-sample max
    magnitude of the terms."""
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), _identity_sizes(name)
    g = torch.Generator(device="cuda").manual_seed(4242 + n)
    q, dq, ddq = (torch.rand((N, n), dtype=torch.float64, device="cuda", generator=g) * 2 - 1 for _ in range(3))
    ddq = 3.0 * ddq
    Dq, Dv, M = chain.getJointTorqueDerivatives(q, dq, ddq, want=("dq", "dv", "M"))   # [s, k, i]
    big = lambda *ts: torch.stack([t.abs().reshape(N, -1).amax(dim=1) for t in ts]).amax(dim=0).clamp_min(1e-300)
    # dtau_dv Dq = 2 (tau_nl(q, Dq) - tau_nl(q, 0)): the velocity term is homogeneous of degree 2
    lhs = torch.einsum("ski,sk->si", Dv, dq)
    h1, h0 = chain.getJointTorqueNonLinearPart(q, dq), chain.getJointTorqueNonLinearPart(q, torch.zeros_like(dq))
    r1 = float(((lhs - 2.0 * (h1 - h0)).abs().amax(dim=1) / big(Dv * dq[:, :, None], h1, h0)).max())
    # M against rdyn_joint_inertia
    M2 = chain.getJointInertia(q)
    r2 = float(((M - M2).abs().reshape(N, -1).amax(dim=1) / big(M2)).max())
    # Dq = DDq = 0: dtau_dq is the Hessian of the potential, symmetric
    zero = torch.zeros_like(q)
    H = chain.getJointTorqueDerivatives(q, zero, zero, want="dq")
    r3 = float(((H - H.transpose(1, 2)).abs().reshape(N, -1).amax(dim=1) / big(H)).max())
    print("%s N=%d: euler %.3g, M %.3g, hessian symmetry %.3g (bounds 1e-11)" % (name, N, r1, r2, r3))
    assert r1 <= 1e-11 and r2 <= 1e-11 and r3 <= 1e-11, (r1, r2, r3)
    # no gravity, Dq = DDq = 0: the torque is zero for every q, and so is dtau_dq -- relative to the magnitude of the same matrix WITH gravity
    from rosdyn_amd import Chain
    xml, base, tool, inputs = _spec(name)
    free = Chain(xml, base, tool, (0.0, 0.0, 0.0))
    if inputs:
        assert free.setInputJointsName(inputs)
    Z = free.getJointTorqueDerivatives(q, zero, zero, want="dq")
    r4 = float((Z.abs().reshape(N, -1).amax(dim=1) / big(H)).max())
    print("%s N=%d: no gravity %.3g (bound 1e-11)" % (name, N, r4))
    assert r4 <= 1e-11, r4
    # directional check against central differences of rdyn_joint_torque at two steps (see the module docstring)
    e, f, gg = (torch.rand((N, n), dtype=torch.float64, device="cuda", generator=g) * 2 - 1 for _ in range(3))
    terms = (torch.einsum("ski,sk->si", Dq, e), torch.einsum("ski,sk->si", Dv, f), torch.einsum("ski,sk->si", M, gg))
    lin = terms[0] + terms[1] + terms[2]
    tau = chain.getJointTorque(q, dq, ddq)
    scale = big(*terms) + tau.abs().amax(dim=1)
    errs = []
    for h in (2.0 ** -7, 2.0 ** -8):
        fd = (chain.getJointTorque(q + h * e, dq + h * f, ddq + h * gg) - chain.getJointTorque(q - h * e, dq - h * f, ddq - h * gg)) / (2.0 * h)
        errs.append((fd - lin).abs().amax(dim=1) / scale)
    sel = errs[0] >= 1e-9
    ratio = errs[0][sel] / errs[1][sel]
    print("%s N=%d: directional err(2^-7) max %.3g (bound 4e-3), err ratio %.4g .. %.4g over %d samples (bounds 3.5, 4.5)"
          % (name, N, float(errs[0].max()), float(ratio.min()), float(ratio.max()), int(sel.sum())))
    assert float(errs[0].max()) <= 4e-3
    assert int(sel.sum()) > N // 2 and float(ratio.min()) >= 3.5 and float(ratio.max()) <= 4.5


def _raw(chain, N, layout, tq, tdq, tddq, pq, pv, pm, stream=None):
    import torch
    from rosdyn_amd._lib import Batch, check, lib
    b = Batch()
    b.n_samples = N
    b.q, b.dq, b.ddq = tq.data_ptr(), tdq.data_ptr(), tddq.data_ptr()
    b.layout = 1 if layout == "element" else 0
    b.device = -1
    b.stream = (stream or torch.cuda.current_stream()).cuda_stream
    check(lib().rdyn_joint_torque_derivatives(chain._h, C.byref(b), pq, pv, pm))


@pytest.mark.parametrize("name", ["ur10_like", "panda_like", "mixed_joints", "ur10_public_long", "rev10", "rev14", "gen20_permuted"])
def test_plumbing_null_outputs_guard_bands_unaligned_output_and_batch_prefix(name):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 1000
    nn = n * n
    q, dq, ddq = _inputs(n, N, seed=11)
    for layout in ("sample", "element"):
        tq, tdq, tddq = _dev(torch, q, layout), _dev(torch, dq, layout), _dev(torch, ddq, layout)
        full = chain.getJointTorqueDerivatives(tq, tdq, tddq, layout=layout, want=("dq", "dv", "M"))
        names = ("dq", "dv", "M")
        # any subset of the outputs leaves the others bit-identical
        for mask in range(1, 7):
            want = tuple(k for b, k in enumerate(names) if mask >> b & 1)
            part = chain.getJointTorqueDerivatives(tq, tdq, tddq, layout=layout, want=want)
            for k, t in zip(want, part):
                assert torch.equal(t, full[names.index(k)]), (layout, want, k)
        # poisoned guard bands; sample-major at an 8-byte (not 128-byte) offset gives the same bits as the aligned call
        G = 24
        bufs = [torch.full((G + 1 + N * nn + G,), 12345.5, dtype=torch.float64, device="cuda") for _ in range(3)]
        outs = [b[G + 1:G + 1 + N * nn] for b in bufs]
        assert all(o.data_ptr() % 128 != 0 and o.data_ptr() % 8 == 0 for o in outs)
        _raw(chain, N, layout, tq, tdq, tddq, *[o.data_ptr() for o in outs])
        torch.cuda.synchronize()
        for o, b, t in zip(outs, bufs, full):
            assert torch.equal(o.view(t.shape), t), layout
            assert (b[:G + 1] == 12345.5).all() and (b[G + 1 + N * nn:] == 12345.5).all()
        # the prefix of a larger batch equals the smaller batch bit for bit
        for Ns in (1, 63, 64, 65, 200):
            sq, sdq, sddq = _dev(torch, q[:Ns], layout), _dev(torch, dq[:Ns], layout), _dev(torch, ddq[:Ns], layout)
            small = chain.getJointTorqueDerivatives(sq, sdq, sddq, layout=layout, want=("dq", "dv", "M"))
            for t, u in zip(small, full):
                assert torch.equal(t, u[:Ns] if layout == "sample" else u[..., :Ns]), (layout, Ns)
    # both layouts agree bit for bit
    a = _derivs(torch, chain, q, dq, ddq, "sample")
    b = _derivs(torch, chain, q, dq, ddq, "element")
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name,perm", [("ur10_like", [3, 0, 5, 1, 4, 2]), ("panda_like", [6, 2, 0, 4, 1, 5, 3]), ("rev14", [13, 0, 7, 3, 9, 1, 12, 5, 2, 11, 4, 10, 6, 8])])
def test_permuted_input_joints_permute_rows_and_columns(name, perm):
    torch = pytest.importorskip("torch")
    chain, moved = _chain(name), _chain(name)
    names = chain.getActiveJointsName()
    assert moved.setInputJointsName([names[p] for p in perm])
    n, N = len(names), 777
    q, dq, ddq = _inputs(n, N, seed=31)
    base = _derivs(torch, chain, q, dq, ddq, "sample")
    got = _derivs(torch, moved, q[:, perm], dq[:, perm], ddq[:, perm], "sample")
    for what, x, y in zip(("dtau_dq", "dtau_dv", "M"), base, got):
        want = x[:, perm][:, :, perm]
        if len(names) <= 10:
            assert np.array_equal(y, want), what   # the same kernel on the same chain joints: the same bits
        else:
            assert _rel(y - want, want) <= 1e-11, what


@pytest.mark.parametrize("name", ["ur10_like", "rev14"])
def test_replays_from_a_captured_graph(name):
    torch = pytest.importorskip("torch")
    chain = _chain(name)
    n, N = chain.getActiveJointsNumber(), 20000
    q, dq, ddq = (torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(3))
    outs = [torch.empty((N, n, n), dtype=torch.float64, device="cuda") for _ in range(3)]
    _raw(chain, N, "sample", q, dq, ddq, *[o.data_ptr() for o in outs])   # first use outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            _raw(chain, N, "sample", q, dq, ddq, *[o.data_ptr() for o in outs], stream=s)
    for k in range(3):
        q.uniform_(-1, 1)
        dq.uniform_(-1, 1)
        ddq.uniform_(-3, 3)
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        again = chain.getJointTorqueDerivatives(q, dq, ddq, want=("dq", "dv", "M"))
        for o, t in zip(outs, again):
            assert torch.equal(o, t)


def test_facade_batch_method_and_single_sample_getter(tmp_path):
    """tests/cpp/torque_derivatives_facade.cpp: getJointTorqueDerivativesBatch and getJointTorqueDerivatives of the C++ facade."""
    exe = tmp_path / "td_facade"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "rosdyn_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "torque_derivatives_facade.cpp"),
                           "-o", str(exe), "-L" + os.path.join(ROOT, "rosdyn_amd"), "-lrdyn_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "rosdyn_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    long_urdf = tmp_path / "rev14.urdf"
    long_urdf.write_text(generated_revolute_chain(14, 1014))
    r = subprocess.run([str(exe), os.path.join(FIXTURES, "ur10_like.urdf"), os.path.join(FIXTURES, "ur10_public.urdf"), str(long_urdf)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
