"""GPU tests of rosdyn_amd.autograd with external link wrenches: loss.backward() reaches q0, Dq0, tau and the wrench tensor, and the
gradients are the direct Chain.getJointAccelerationVjp(ext_wrenches=) / Chain.rolloutAdjoint(ext_wrenches=) results, bit for bit -- for a
wrench held over the horizon (its gradient the sum over the steps) and for one record per step.  torch.autograd.gradcheck at its default
tolerances compares the backward with central differences of the wrappers' own forward calls."""
import pytest

from _arrays import AUTOGRAD_DT as DT, AUTOGRAD_N as N, AUTOGRAD_T as T, INTEGRATORS, TAU_SCALE, _leaves
from _chains import _chain
from _components import _autograd_components as _components

pytestmark = pytest.mark.gpu


def _wrench_leaf(torch, name, chain, layout="sample", link=None, steps=None, seed=12000):
    """every link: (N, L, 6) / (L * 6, N); one link: (N, 6) / (6, N); with steps a leading axis"""
    from rosdyn_amd.samples import uniform_pm1
    L = chain.getLinksNumber()
    rec = (N, L, 6) if link is None else (N, 6)
    if layout == "element":
        rec = (rec[-1] * (L if link is None else 1), N)
    shape = rec if steps is None else (steps,) + rec
    w = TAU_SCALE[name] * uniform_pm1(seed, (int(__import__("numpy").prod(shape)),)).reshape(shape)
    return torch.from_numpy(w).cuda().requires_grad_(True)


@pytest.mark.parametrize("link", [None, "tool"], ids=["every_link", "tool"])
@pytest.mark.parametrize("name", ["planar_2r", "ur10_like"])
def test_gradcheck_joint_acceleration_with_wrenches(name, link):
    torch = pytest.importorskip("torch")
    from rosdyn_amd import autograd
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    lname = None if link is None else chain.getLinksName()[-1]
    q, dq, tau = _leaves(torch, name, n, seed=12100)
    w = _wrench_leaf(torch, name, chain, link=link, seed=12103)
    fn = lambda a, b, c, d: autograd.joint_acceleration(chain, a, b, c, ext_wrenches=d, ext_link=lname)
    assert torch.autograd.gradcheck(fn, (q, dq, tau, w))


@pytest.mark.parametrize("held", [True, False], ids=["held", "per_step"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", ["planar_2r", "ur10_like"])
def test_gradcheck_rollout_with_wrenches(name, integrator, held):
    torch = pytest.importorskip("torch")
    from rosdyn_amd import autograd
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    q0, dq0, tau = _leaves(torch, name, n, steps=T, seed=12200)
    w = _wrench_leaf(torch, name, chain, steps=None if held else T, seed=12203)
    fn = lambda a, b, c, d: autograd.rollout(chain, a, b, c, DT, integrator=integrator, trajectory=True, ext_wrenches=d)
    assert len(fn(q0, dq0, tau, w)) == 4
    assert torch.autograd.gradcheck(fn, (q0, dq0, tau, w))


@pytest.mark.parametrize("layout", ["sample", "element"])
@pytest.mark.parametrize("with_components", [False, True], ids=["plain", "components"])
def test_joint_acceleration_backward_gives_the_product_own_bits(with_components, layout):
    torch = pytest.importorskip("torch")
    from rosdyn_amd import autograd
    name = "ur10_like"
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    cs = _components(n) if with_components else None
    for link in (None, chain.getLinksName()[-1], chain.getLinksName()[3]):
        q, dq, tau = _leaves(torch, name, n, seed=12300)
        if layout == "element":
            q, dq, tau = (t.detach().T.contiguous().requires_grad_(True) for t in (q, dq, tau))
        w = _wrench_leaf(torch, name, chain, layout, link=link, seed=12303)
        ddq = autograd.joint_acceleration(chain, q, dq, tau, components=cs, layout=layout, ext_wrenches=w, ext_link=link)
        seed = torch.rand_like(ddq)
        (seed * ddq).sum().backward()
        d = lambda t: t.detach()
        fwd, st = chain.getJointAcceleration(d(q), d(dq), d(tau), layout=layout, components=cs, ext_wrenches=d(w), ext_link=link)
        assert torch.equal(fwd, d(ddq)) and bool((st == 1).all())
        r = chain.getJointAccelerationVjp(d(q), d(dq), d(tau), seed, layout=layout, want=("q", "dq", "tau", "ext"), components=cs,
                                          ext_wrenches=d(w), ext_link=link)
        assert bool((r[0] == 1).all())
        for leaf, g in zip((q, dq, tau, w), r[1:]):
            assert leaf.grad.shape == leaf.shape and torch.equal(leaf.grad, g) and bool(g.abs().sum() > 0)
        # only the wrench needs a gradient
        w2 = d(w).clone().requires_grad_(True)
        (seed * autograd.joint_acceleration(chain, d(q), d(dq), d(tau), components=cs, layout=layout, ext_wrenches=w2, ext_link=link)).sum().backward()
        assert torch.equal(w2.grad, r[4])


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("layout", ["sample", "element"])
def test_rollout_backward_gives_the_adjoint_call_own_bits(integrator, layout):
    torch = pytest.importorskip("torch")
    from rosdyn_amd import autograd
    name = "ur10_like"
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    cs = _components(n)
    d = lambda t: t.detach()
    for link in (None, chain.getLinksName()[-1]):
        for steps in (None, T):   # a wrench held over the horizon; one record per step
            q0, dq0, tau = _leaves(torch, name, n, steps=T, seed=12400)
            if layout == "element":
                q0, dq0 = (t.detach().T.contiguous().requires_grad_(True) for t in (q0, dq0))
                tau = tau.detach().transpose(1, 2).contiguous().requires_grad_(True)
            w = _wrench_leaf(torch, name, chain, layout, link=link, steps=steps, seed=12403)
            q_end, dq_end, q_traj, dq_traj = autograd.rollout(chain, q0, dq0, tau, DT, integrator=integrator, trajectory=True, components=cs,
                                                              layout=layout, ext_wrenches=w, ext_link=link)
            cq, cv, rq = torch.rand_like(q_end), torch.rand_like(dq_end), torch.rand_like(q_traj)
            ((cq * q_end).sum() + (cv * dq_end).sum() + (rq * q_traj).sum()).backward()
            r = chain.rollout(d(q0), d(dq0), d(tau), DT, integrator=integrator, layout=layout, trajectory_every=1, components=cs,
                              ext_wrenches=d(w), ext_link=link)
            assert torch.equal(r[0], d(q_end)) and torch.equal(r[3], d(q_traj)) and bool((r[2] == 1).all())
            g = chain.rolloutAdjoint(d(q0), d(dq0), d(tau), DT, r[3], r[4], gq_end=cq, gDq_end=cv, gq_traj=rq, gDq_traj=torch.zeros_like(rq),
                                     integrator=integrator, layout=layout, components=cs, ext_wrenches=d(w), ext_link=link, want_ext=True,
                                     sum_ext=steps is None)
            assert bool((g[3] == 1).all())
            assert torch.equal(q0.grad, g[0]) and torch.equal(dq0.grad, g[1]) and torch.equal(tau.grad, g[2])
            assert w.grad.shape == w.shape and torch.equal(w.grad, g[4]) and bool(w.grad.abs().sum() > 0)
    # a wrench sequence longer than the horizon: the records that are not read get a zero gradient
    q0, dq0, tau = _leaves(torch, name, n, steps=T, seed=12500)
    if layout == "sample":
        w = _wrench_leaf(torch, name, chain, steps=T + 2, seed=12503)
        q_end, _ = autograd.rollout(chain, q0, dq0, tau, DT, integrator=integrator, ext_wrenches=w)
        q_end.sum().backward()
        assert w.grad.shape == w.shape and bool((w.grad[T:] == 0).all()) and bool(w.grad[:T].abs().sum() > 0)


def test_wrenches_with_parameters_raise_and_a_failed_sample_is_nan_alone():
    torch = pytest.importorskip("torch")
    from rosdyn_amd import autograd
    name = "ur10_like"
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    q, dq, tau = _leaves(torch, name, n, steps=T, seed=12600)
    w = _wrench_leaf(torch, name, chain, seed=12603)
    pi = torch.from_numpy(chain.getNominalParameters()).requires_grad_(True)
    with pytest.raises(ValueError, match="follow-up"):
        autograd.rollout(chain, q, dq, tau, DT, ext_wrenches=w, parameters=pi)
    with pytest.raises(ValueError, match="follow-up"):
        autograd.joint_acceleration(chain, q, dq, tau[0], ext_wrenches=w, parameters=pi)
    with pytest.raises(ValueError, match="follow-up"):
        autograd.joint_acceleration(chain, q, dq, tau[0], ext_wrenches=w, components=_components(n), component_parameters=torch.zeros(7, dtype=torch.float64))
    # a NaN wrench entry: that sample's gradients are NaN, the others finite
    with torch.no_grad():
        w[1, 3, 2] = float("nan")
    ddq = autograd.joint_acceleration(chain, q, dq, tau[0], ext_wrenches=w)
    assert bool(torch.isnan(ddq[1]).all()) and bool(torch.isfinite(ddq[[0, 2]]).all())
    torch.nan_to_num(ddq, nan=0.0).sum().backward()   # (a finite loss: the NaN comes from the backward call itself)
    for t in (q, dq, w):
        assert bool(torch.isnan(t.grad[1]).all()) and bool(torch.isfinite(t.grad[[0, 2]]).all())
