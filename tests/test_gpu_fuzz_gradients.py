"""Seeded structural fuzz (-m gpu) of the six entry points merged after test_gpu_fuzz_dynamics.py: forward dynamics and rollouts with
friction and spring components, rdyn_forward_dynamics_derivatives, rdyn_forward_dynamics_vjp and rdyn_rollout_adjoint, on that module's
64 chains -- the same chain, gravity, input subset, layout and inputs per seed (Case, imported, not copied; RDYN_FUZZ_OFFSET moves the
seeds as it does there), N = 257, T = 4, dt = 1e-3.  Every chain has 1 .. 10 chain joints: the register kernels k_fwd_dyn_deriv,
k_fwd_dyn_vjp, k_rollout_adjoint <1> .. <10> and the forward kernels with components; the chunked route (11 .. 32 joints) is not fuzzed here.
Every bound holds per sample, no sample is excused; a seed is regular or singular by classify() of the oracle's inertia alone.

Components per seed: fuzz_specs(c) -- the five-entry list of test_gpu_forward_dynamics_derivatives.py (min_velocity 0.3, max_velocity
0.8), reduced for n = 1 and n = 2 the way test_gpu_rollout_components.py reduces its list (no FRICTION2 on the last joint for n = 1, no
spring on joint 1 below n = 3), every parameter times s = 2^floor(log2(min over samples and joints of diag M_ref)) (s = 1 where that
minimum is not positive: a singular seed).  Joint indices are INPUT indices: on a permuted subset chain joint 0 is the first selected joint,
wherever it sits in the chain.  tests/test_fuzz_gradients_inputs.py pins, without a GPU, what these tests rest on.

No tolerance here is new; each is the one of the module its check is imported from:
  forward dynamics + components   the residual bound of test_gpu_forward_dynamics.py (1e-11) with h_ref + tau_c_ref for h_ref, tau_c_ref
                                  from oracle.components_regressor and its norm added to the scale; the plain call must miss that bound
  rollouts + components           the end state against the numpy rollout over the oracle with components within rollout_bound_c() =
                                  8 dev, computed at run time from the oracle alone (rollout_bound of test_gpu_fuzz_dynamics.py over
                                  _oracle_fd_c); [1, 3] steps give the same bits; the rollout without components must miss the bound
  derivatives                     _residual_ratios of test_gpu_forward_dynamics_derivatives.py <= 1e-11 (the closed-form _slopes on the
                                  reference diagonals; without them > 1e-6); ddq is getJointAcceleration's, minv symmetric, every `want`
                                  subset the full call's, all bitwise
  VJP                             _residual_ratios of test_gpu_forward_dynamics_vjp.py <= 1e-11; the other layout and tau_bar written
                                  over the seed give the same bits.  The exact reference at the library's ddq is computed once per
                                  (seed, with or without components) and shared by the derivative and the VJP test, which first
                                  assert that their two calls returned the same ddq bits
  rollout adjoint                 one step against the library's own product composed in numpy, 1e-11 of the sum of the absolute terms
                                  (test_gpu_rollout_adjoint.py); T = 4 with running seeds: [1, 3] steps give the whole call's bits and
                                  sum_tau its 4 eps sum|terms|.  With the VJP test this pins every multi-step gradient to the oracle.
  singular seeds                  every entry point reports -1 and NaN in every output on all 257 samples; a regular chain evaluated
                                  afterwards in the same process is clean
The exact reference costs a fraction of a second per seed at these sizes, so all 257 samples enter every residual."""
import numpy as np
import pytest

from _arrays import (DERIVATIVE_NAMES, EPS, INTEGRATORS, VJP_NAMES, _adjoint, _derivatives_call, _dev,
                     _dev_seq, _forward, _host, _inf, _rollout, _seeds, _solve, _vjp_call)
from _components import _set, _slopes as _component_slopes
from _fuzz import DT, N, T, _chain, _get, _regular_neighbour, component_torque_ref, fuzz_specs, rollout_bound_c, seed_class
from _references import (_cached_reference, _derivative_residual_ratios, _input_types, _lib_abs_vjp,
                         _lib_fd, _lib_vjp, _np_step_adjoint, _vjp_residual_ratios)

pytestmark = pytest.mark.gpu
COMPONENTS = pytest.mark.parametrize("with_components", [False, True], ids=["plain", "components"])
SEEDS = pytest.mark.parametrize("seed", range(64))


def _what(c, *more):
    return "seed %d %s(nJ %d, n %d, %s, %s)" % (c.seed, "".join(m + " " for m in more), c.ref.nJ, c.n, "subset" if c.inputs else "all inputs", c.layout)


def _cs(c, with_components=True):
    return _set(fuzz_specs(c), c.n) if with_components else None


def _other(layout):
    return "element" if layout == "sample" else "sample"


# ---- a. forward dynamics with components
def _forward_dynamics_c_regular(torch, c, chain, what):
    tau_c = component_torque_ref(c)
    ddq, st = _solve(torch, chain, c.q, c.dq, c.tau, c.layout, components=_cs(c))
    assert st.shape == (N,) and (st == 1).all(), np.unique(st)
    assert ddq.shape == (N, c.n) and np.isfinite(ddq).all()
    residual = lambda a: _inf(np.einsum("sij,sj->si", c.M, a) + c.h + tau_c - c.tau)
    scale_of = lambda a: np.abs(c.M).sum(axis=2).max(axis=1) * _inf(a) + _inf(c.tau) + _inf(c.h) + _inf(tau_c)
    ratio = residual(ddq) / scale_of(ddq)
    plain, stp = _solve(torch, chain, c.q, c.dq, c.tau, c.layout)
    assert (stp == 1).all()
    bare = residual(plain) / scale_of(plain)
    print("%s: residual ratio max %.3g (bound 1e-11), without components %.3g" % (what, ratio.max(), bare.max()))
    assert (ratio <= 1e-11).all(), (float(ratio.max()), int(np.argmax(ratio)))
    assert (bare > 1e-11).any(), "the components matter at this bound"


@SEEDS
def test_forward_dynamics_with_components(seed):
    torch = pytest.importorskip("torch")
    c = _get(seed)
    kind = seed_class(c)
    chain = _chain(c)
    if kind == "regular":
        _forward_dynamics_c_regular(torch, c, chain, _what(c))
        return
    ddq, st = _solve(torch, chain, c.q, c.dq, c.tau, c.layout, components=_cs(c))
    assert st.shape == (N,) and (st == -1).all(), np.unique(st)
    assert ddq.shape == (N, c.n) and np.isnan(ddq).all()
    print("%s: singular, status -1 and NaN on all %d samples" % (_what(c), N))
    good = _regular_neighbour(seed)
    _forward_dynamics_c_regular(torch, good, _chain(good), "seed %d after the singular seed %d" % (good.seed, seed))


# ---- b. rollouts with components
@SEEDS
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_rollout_with_components(seed, integrator):
    torch = pytest.importorskip("torch")
    c = _get(seed)
    kind = seed_class(c)
    chain = _chain(c)
    cs = _cs(c)
    what = _what(c, integrator)
    if kind == "singular":
        q1, dq1, st, qt, dqt = _rollout(torch, chain, c.q, c.dq, c.tau_seq, DT, integrator, c.layout, trajectory_every=1, components=cs)
        assert st.shape == (N,) and (st == -1).all(), np.unique(st)
        assert q1.shape == (N, c.n) and np.isnan(q1).all() and np.isnan(dq1).all()
        assert qt.shape == (T, N, c.n) and np.isnan(qt).all() and np.isnan(dqt).all()
        print("%s: singular, status -1 and NaN in the end state and all %d records" % (what, T))
        return
    bound, dev, qr, dqr = rollout_bound_c(c, integrator)
    assert np.isfinite(bound) and bound > 0.0
    q1, dq1, st = _rollout(torch, chain, c.q, c.dq, c.tau_seq, DT, integrator, c.layout, components=cs)
    assert st.shape == (N,) and (st == 1).all(), np.unique(st)
    scale = np.maximum(1.0, np.maximum(_inf(qr), _inf(dqr)))
    err = np.maximum(_inf(q1 - qr), _inf(dq1 - dqr)) / scale
    qn, dqn, stn = _rollout(torch, chain, c.q, c.dq, c.tau_seq, DT, integrator, c.layout, components=None)
    bare = np.maximum(_inf(qn - qr), _inf(dqn - dqr)) / scale
    print("%s: end-state err max %.3g (run-time bound %.3g = 8 x %.3g), ratio %.3g; without components %.3g"
          % (what, err.max(), bound, dev, err.max() / bound, bare.max()))
    assert (err <= bound).all(), (float(err.max()), bound, int(np.argmax(err)))
    assert (stn == 1).all() and (bare > bound).any(), "the components matter at this bound"
    # the horizon cut into [1, 3] steps: the same bits
    qa, dqa, sta = _rollout(torch, chain, c.q, c.dq, c.tau_seq[:1], DT, integrator, c.layout, components=cs)
    qb, dqb, stb = _rollout(torch, chain, qa, dqa, c.tau_seq[1:], DT, integrator, c.layout, components=cs)
    assert np.array_equal(qb, q1) and np.array_equal(dqb, dq1) and np.array_equal(np.minimum(sta, stb), st)


# ---- c, d. the exact reference at the library's ddq, once per (seed, with or without components)
def _shared_reference(c, with_components, types, ddq):
    """(M_ref, Dq_ref, Dv_ref, tau_ref, gscale), read-only; asserts the construction gap (1e-12) when it builds the reference and, on
    every call, that ddq has the bits the reference was built at"""
    assert types == c.oracle_types()
    return _cached_reference(("fuzz", c.data_seed, bool(with_components)), c.ref, types, c.q, c.dq, ddq)


def _slopes(c, with_components):
    return _component_slopes(fuzz_specs(c), c.q, c.dq) if with_components else None


# ---- c. forward-dynamics derivatives
def _derivatives_regular(torch, c, chain, with_components, what):
    cs = _cs(c, with_components)
    n = c.n
    full = _derivatives_call(torch, chain, c.q, c.dq, c.tau, c.layout, components=cs)
    ddq, st, Xq, Xv, Minv = full
    assert st.shape == (N,) and (st == 1).all(), np.unique(st)
    assert ddq.shape == (N, n) and all(X.shape == (N, n, n) and np.isfinite(X).all() for X in (Xq, Xv, Minv))
    want, st2 = _solve(torch, chain, c.q, c.dq, c.tau, c.layout, components=cs)
    assert np.array_equal(want, ddq) and (st2 == 1).all(), "ddq is getJointAcceleration's, bitwise"
    types = _input_types(chain)
    cached = _shared_reference(c, with_components, types, ddq)
    slopes = _slopes(c, with_components)
    worst = _derivative_residual_ratios(c.ref, types, c.q, c.dq, ddq, Xq, Xv, Minv, slopes=slopes, cached=cached)
    print("%s: worst residual ratio dddq_dq %.3g dddq_dv %.3g minv %.3g (bound 1e-11)" % (what, worst["dddq_dq"], worst["dddq_dv"], worst["minv"]))
    for k, r in worst.items():
        assert r <= 1e-11, (k, r)
    if with_components:
        # the slopes matter at this bound, and land on the right diagonal entry: without them the residual is far off
        bare = _derivative_residual_ratios(c.ref, types, c.q, c.dq, ddq, Xq, Xv, Minv, cached=cached)
        print("%s: without the slopes dddq_dq %.3g dddq_dv %.3g (must exceed 1e-6)" % (what, bare["dddq_dq"], bare["dddq_dv"]))
        must = [k for k, sl in zip(("dddq_dq", "dddq_dv"), slopes) if n >= 2 or np.abs(sl).max() > 0.0]
        assert must and all(bare[k] > 1e-6 for k in must), (must, bare)
    assert np.array_equal(Minv, np.swapaxes(Minv, 1, 2)), "minv: the same bits in both triangles"
    for mask in range(1, 7):
        names = tuple(k for b, k in enumerate(DERIVATIVE_NAMES) if mask >> b & 1)
        part = _derivatives_call(torch, chain, c.q, c.dq, c.tau, c.layout, want=names, components=cs)
        assert np.array_equal(part[0], ddq) and np.array_equal(part[1], st)
        for k, t in zip(names, part[2:]):
            assert np.array_equal(t, full[2 + DERIVATIVE_NAMES.index(k)]), (names, k)


@SEEDS
@COMPONENTS
def test_forward_dynamics_derivatives(seed, with_components):
    torch = pytest.importorskip("torch")
    c = _get(seed)
    kind = seed_class(c)
    chain = _chain(c)
    what = _what(c, "components" if with_components else "plain")
    if kind == "regular":
        _derivatives_regular(torch, c, chain, with_components, what)
        return
    for names in (DERIVATIVE_NAMES, ("dv",)):
        out = _derivatives_call(torch, chain, c.q, c.dq, c.tau, c.layout, want=names, components=_cs(c, with_components))
        assert out[1].shape == (N,) and (out[1] == -1).all(), np.unique(out[1])
        assert out[0].shape == (N, c.n) and np.isnan(out[0]).all()
        assert all(X.shape == (N, c.n, c.n) and np.isnan(X).all() for X in out[2:])
    print("%s: singular, status -1 and NaN in ddq and all three matrices on all %d samples" % (what, N))
    good = _regular_neighbour(seed)
    _derivatives_regular(torch, good, _chain(good), with_components, "seed %d after the singular seed %d" % (good.seed, seed))


# ---- d. the reverse-mode product
@SEEDS
@COMPONENTS
def test_forward_dynamics_vjp(seed, with_components):
    torch = pytest.importorskip("torch")
    from rosdyn_amd.samples import uniform_pm1
    c = _get(seed)
    kind = seed_class(c)
    chain = _chain(c)
    cs = _cs(c, with_components)
    what = _what(c, "components" if with_components else "plain")
    a = uniform_pm1(c.data_seed + 5, (N, c.n))
    every = VJP_NAMES + ("ddq",)
    full = _vjp_call(torch, chain, c.q, c.dq, c.tau, a, c.layout, components=cs)
    st, qb, vb, tb, ddq = full
    assert st.shape == (N,) and all(x.shape == (N, c.n) for x in full[1:])
    if kind == "singular":
        assert (st == -1).all(), np.unique(st)
        assert all(np.isnan(x).all() for x in full[1:])
        other = _vjp_call(torch, chain, c.q, c.dq, c.tau, a, _other(c.layout), want=("tau",), components=cs)
        assert (other[0] == -1).all() and np.isnan(other[1]).all()
        print("%s: singular, status -1 and NaN in every output on all %d samples" % (what, N))
        return
    assert (st == 1).all(), np.unique(st)
    assert all(np.isfinite(x).all() for x in full[1:])
    cached = _shared_reference(c, with_components, _input_types(chain), ddq)   # asserts: the derivative call's ddq bits
    worst = _vjp_residual_ratios(cached, a, qb, vb, tb, slopes=_slopes(c, with_components))
    print("%s: worst residual ratio tau_bar %.3g q_bar %.3g dq_bar %.3g (bound 1e-11)" % (what, worst["tau_bar"], worst["q_bar"], worst["dq_bar"]))
    for k, r in worst.items():
        assert r <= 1e-11, (k, r)
    # the other layout: the same bits
    for x, y in zip(full, _vjp_call(torch, chain, c.q, c.dq, c.tau, a, _other(c.layout), components=cs)):
        assert np.array_equal(x, y)
    # tau_bar written over the seed, alone and with the other products: the same bits
    dev = lambda x: _dev(torch, x, c.layout)
    for names in (("tau",), VJP_NAMES):
        ta = dev(a)
        out = chain.getJointAccelerationVjp(dev(c.q), dev(c.dq), dev(c.tau), ta, layout=c.layout, want=names, out={"tau": ta}, components=cs)
        assert out[1 + names.index("tau")].data_ptr() == ta.data_ptr() and np.array_equal(out[0].cpu().numpy(), st)
        for k, t in zip(names, out[1:]):
            assert np.array_equal(_host(t, c.layout), full[1 + every.index(k)]), (names, k)


# ---- e. the rollout adjoint
def _adjoint_seeds(c, steps):
    """end seeds (N, n) x 2 and running seeds (steps, N, n) x 2 of test_gpu_rollout_adjoint.py, away from the seeds of the case's inputs"""
    return _seeds(c.n, N, steps, seed=100000 + c.data_seed)


def _adjoint_singular(torch, c, chain, cs, integrator, steps, what):
    gq, gv, rq, rv = _adjoint_seeds(c, steps)
    fw, st = _forward(torch, chain, c.q, c.dq, c.tau_seq[:steps], DT, integrator, c.layout, components=cs)
    assert st.shape == (N,) and (st == -1).all(), np.unique(st)
    assert bool(torch.isnan(fw[3]).all()) and bool(torch.isnan(fw[4]).all()) and fw[3].shape[0] == steps
    for kw in ({}, {"sum_tau": True}):
        r = _adjoint(torch, chain, fw, DT, integrator, c.layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, components=cs, **kw)
        assert r[3].shape == (N,) and (r[3] == -1).all(), np.unique(r[3])
        assert r[0].shape == (N, c.n) and np.isnan(r[0]).all() and np.isnan(r[1]).all()
        assert r[2].shape == ((N, c.n) if kw else (steps, N, c.n)) and np.isnan(r[2]).all()
    print("%s: singular, the forward call and the adjoint report -1 and NaN in every output (%d steps)" % (what, steps))
    good = _regular_neighbour(c.seed)
    gcs = _cs(good, cs is not None)
    gchain = _chain(good)
    fw, st = _forward(torch, gchain, good.q, good.dq, good.tau_seq[:steps], DT, integrator, good.layout, components=gcs)
    gq, gv, rq, rv = _adjoint_seeds(good, steps)
    r = _adjoint(torch, gchain, fw, DT, integrator, good.layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, components=gcs)
    assert (st == 1).all() and (r[3] == 1).all() and all(np.isfinite(x).all() for x in r[:3])


@SEEDS
@pytest.mark.parametrize("integrator", INTEGRATORS)
@COMPONENTS
def test_rollout_adjoint_one_step_against_the_library_own_product(seed, integrator, with_components):
    """test_one_step_against_the_library_own_product of test_gpu_rollout_adjoint.py on the fuzz chain with c.q, c.dq, c.tau_seq[:1]."""
    torch = pytest.importorskip("torch")
    c = _get(seed)
    kind = seed_class(c)
    chain = _chain(c)
    cs = _cs(c, with_components)
    what = _what(c, integrator, "components" if with_components else "plain")
    if kind == "singular":
        _adjoint_singular(torch, c, chain, cs, integrator, 1, what)
        return
    fd, vjp, avjp = _lib_fd(torch, chain, cs), _lib_vjp(torch, chain, cs), _lib_abs_vjp(torch, chain, cs)
    q0, dq0, tau = c.q, c.dq, c.tau_seq[:1]
    gq, gv, _, _ = _adjoint_seeds(c, 1)
    want = _np_step_adjoint(vjp, fd, q0, dq0, tau[0], gq, gv, DT, integrator)
    mag = _np_step_adjoint(avjp, fd, q0, dq0, tau[0], np.abs(gq), np.abs(gv), DT, integrator)
    got = None
    for layout in (c.layout, _other(c.layout)):
        fw = (_dev(torch, q0, layout), _dev(torch, dq0, layout), _dev_seq(torch, tau, layout), None, None)
        r = _adjoint(torch, chain, fw, DT, integrator, layout, gq_end=gq, gdq_end=gv, components=cs)
        assert r[3].shape == (N,) and (r[3] == 1).all(), np.unique(r[3])
        if got is not None:
            assert all(np.array_equal(x, y) for x, y in zip(got, r)), "the layouts give the same bits"
        got = r
    worst = {}
    for k, g, w, m in zip(("gq0", "gdq0", "gtau"), (got[0], got[1], got[2][0]), want, mag):
        assert g.shape == (N, c.n) and np.isfinite(g).all() and (m > 0).all()
        worst[k] = float((np.abs(g - w) / m).max())
    print("%s: worst distance / sum of absolute terms gq0 %.3g gdq0 %.3g gtau %.3g (bound 1e-11)" % (what, worst["gq0"], worst["gdq0"], worst["gtau"]))
    for k, r in worst.items():
        assert r <= 1e-11, (k, r)


@SEEDS
@pytest.mark.parametrize("integrator", INTEGRATORS)
@COMPONENTS
def test_rollout_adjoint_split_horizon_and_summed_torque_gradient(seed, integrator, with_components):
    """T = 4, running seeds on every record, gtau per step: the horizon split into [1, 3] steps gives the whole call's bits (the later part
    first, its result the earlier part's end seeds); sum_tau=True within 4 eps sum|terms| of the exactly rounded sum of the per-step gradients (T - 1 = 3
    roundings of eps / 2 of the partial sums, test_gpu_rollout_adjoint.py)."""
    torch = pytest.importorskip("torch")
    c = _get(seed)
    kind = seed_class(c)
    chain = _chain(c)
    cs = _cs(c, with_components)
    what = _what(c, integrator, "components" if with_components else "plain")
    if kind == "singular":
        _adjoint_singular(torch, c, chain, cs, integrator, T, what)
        return
    layout = c.layout
    gq, gv, rq, rv = _adjoint_seeds(c, T)
    fw, st = _forward(torch, chain, c.q, c.dq, c.tau_seq, DT, integrator, layout, components=cs)
    assert (st == 1).all(), np.unique(st)
    tq, tdq, ttau, q_traj, dq_traj = fw
    whole = _adjoint(torch, chain, fw, DT, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, components=cs)
    assert (whole[3] == 1).all() and all(np.isfinite(x).all() for x in whole[:3])
    assert whole[2].shape == (T, N, c.n) and not np.array_equal(whole[0], gq)
    cut = 1
    later = (q_traj[cut - 1], dq_traj[cut - 1], ttau[cut:], q_traj[cut:], dq_traj[cut:])
    b = _adjoint(torch, chain, later, DT, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq[cut:], gdq_traj=rv[cut:], components=cs)
    earlier = (tq, tdq, ttau[:cut], q_traj[:cut], dq_traj[:cut])
    a = _adjoint(torch, chain, earlier, DT, integrator, layout, gq_end=b[0], gdq_end=b[1], gq_traj=rq[:cut], gdq_traj=rv[:cut], components=cs)
    assert np.array_equal(a[0], whole[0]) and np.array_equal(a[1], whole[1])
    assert np.array_equal(np.concatenate([a[2], b[2]]), whole[2])
    assert (a[3] == 1).all() and (b[3] == 1).all()
    tot = _adjoint(torch, chain, fw, DT, integrator, layout, gq_end=gq, gdq_end=gv, gq_traj=rq, gdq_traj=rv, components=cs, sum_tau=True)
    assert tot[2].shape == (N, c.n) and np.array_equal(tot[0], whole[0]) and np.array_equal(tot[1], whole[1]) and (tot[3] == 1).all()
    exact = whole[2].astype(np.longdouble).sum(axis=0)
    terms = np.abs(whole[2]).sum(axis=0)
    ratio = float((np.abs(tot[2] - exact) / (EPS * terms)).max())
    print("%s: [1, 3] steps bitwise; summed torque gradient %.3g eps sum|terms| (bound 4)" % (what, ratio))
    assert (np.abs(tot[2] - exact) <= 4 * EPS * terms).all(), ratio
