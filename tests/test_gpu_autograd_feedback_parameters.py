"""GPU tests of rosdyn_amd.autograd.closed_loop_rollout: loss.backward() through the closed loop with the model among the inputs fills the
gradients of `parameters` and `component_parameters` with the bits of Chain.rolloutParameterAdjoint(feedback=), the gradients of the state,
the feed-forward torques and the law's tensors with the bits autograd.rollout(feedback=) gives on that model, and without parameters it is
autograd.rollout(feedback=)."""
import numpy as np
import pytest

from _arrays import DT, _seeds, _wrench_rollout_inputs as _inputs
from _chains import _chain
from _components import _set, _specs
from _feedback_adjoint import _law

pytestmark = pytest.mark.gpu
MODES = [("semi_implicit_euler", True), ("rk4", True), ("rk4", False)]
MODE_IDS = ["euler", "rk4-hold", "rk4-continuous"]
NAMES = ("q_ref", "Dq_ref", "kp", "kd", "tau_limit")


def _model(torch, chain, n, device):
    """(components, pi, p): the chain's parameters moved by a few percent, as leaves on `device`"""
    cs = _set(_specs(n), n)
    rng = np.random.default_rng(17)
    pi0 = chain.getNominalParameters()
    pi = torch.tensor(pi0 * (1.0 + 0.05 * rng.uniform(-1, 1, pi0.shape)), dtype=torch.float64, device=device, requires_grad=True)
    p0 = np.array(cs.getNominalParameters())
    p = torch.tensor(p0 * (1.0 + 0.05 * rng.uniform(-1, 1, p0.shape)), dtype=torch.float64, device=device, requires_grad=True)
    return cs, pi, p


def _leaves(torch, name, n, N, T, seed):
    q0, dq0, tau = _inputs(name, n, N, T, seed=seed)
    law = _law(name, n, N, T, seed, limits=True, q0=q0, dq0=dq0, tau=tau)
    leaf = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda().requires_grad_(True)
    return tuple(leaf(x) for x in (q0, dq0, tau, law.q_ref, law.dq_ref, law.kp, law.kd, law.lim))


@pytest.mark.parametrize("device", ["cpu", "cuda"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["ur10_like", "ur10_public_long"])
def test_backward_through_the_closed_loop_fills_every_gradient(name, mode, device):
    torch = pytest.importorskip("torch")
    from rosdyn_amd import Feedback, autograd
    integrator, hold = mode
    chain = _chain(name)
    n, N, T = chain.getActiveJointsNumber(), 65, 4
    cs, pi, p = _model(torch, chain, n, device)
    a = _leaves(torch, name, n, N, T, 15100)
    tq, tdq, ttau, q_ref, dq_ref, kp, kd, lim = a
    cq, cv, ct, cu = (torch.from_numpy(x).cuda() for x in _seeds(n, N, T, seed=15100))
    fb = Feedback(q_ref, kp, kd, dq_ref, hold=hold, tau_limit=lim, command_trajectory=True)
    q_end, dq_end, q_traj, dq_traj, u = autograd.closed_loop_rollout(chain, tq, tdq, ttau, DT, fb, integrator=integrator, trajectory=True,
                                                                     components=cs, parameters=pi, component_parameters=p)
    ((cq * q_end).sum() + (cv * dq_end).sum() + (ct * q_traj).sum() + (cu * u).sum()).backward()
    assert pi.grad.device == pi.device and p.grad.device == p.device and pi.grad.shape == pi.shape and p.grad.shape == p.shape
    assert all(t.grad is not None and tuple(t.grad.shape) == tuple(t.shape) and bool(torch.isfinite(t.grad).all()) and bool(t.grad.abs().sum() > 0)
               for t in a)
    # the direct call on the same model: gpi, gcomp bit for bit
    det = lambda t: t.detach()
    chain2, cs2 = chain.withParameters(pi.detach().cpu().numpy()), cs.withParameters(p.detach().cpu().tolist())
    fbd = Feedback(det(q_ref), det(kp), det(kd), det(dq_ref), hold=hold, tau_limit=det(lim), command_trajectory=True)
    r = chain2.rollout(det(tq), det(tdq), det(ttau), DT, integrator=integrator, trajectory_every=1, components=cs2, feedback=fbd)
    assert bool((r[2] == 1).all()) and torch.equal(r[0], q_end) and torch.equal(r[1], dq_end) and torch.equal(r[3], q_traj) and torch.equal(r[5], u)
    g = chain2.rolloutParameterAdjoint(det(tq), det(tdq), det(ttau), DT, r[3], r[4], gq_end=cq, gDq_end=cv, gq_traj=ct, integrator=integrator,
                                       components=cs2, feedback=fbd, want_feedback=NAMES, gu_traj=cu)
    assert torch.equal(pi.grad.cuda(), g[3]) and torch.equal(p.grad.cuda(), g[4]) and bool(g[3].abs().sum() > 0) and bool(g[4].abs().sum() > 0)
    # the state's and the law's gradients: autograd.rollout(feedback=) on that model, bit for bit
    b = tuple(t.detach().clone().requires_grad_() for t in a)
    fb2 = Feedback(b[3], b[5], b[6], b[4], hold=hold, tau_limit=b[7], command_trajectory=True)
    e = autograd.rollout(chain2, b[0], b[1], b[2], DT, integrator=integrator, trajectory=True, components=cs2, feedback=fb2)
    ((cq * e[0]).sum() + (cv * e[1]).sum() + (ct * e[2]).sum() + (cu * e[4]).sum()).backward()
    for x, y in zip(a, b):
        assert torch.equal(x.grad, y.grad)
    # one of the two alone
    pi.grad = None
    out = autograd.closed_loop_rollout(chain, det(tq), det(tdq), det(ttau), DT, fbd, integrator=integrator, components=cs2, parameters=pi)
    assert len(out) == 3
    ((cq * out[0]).sum() + (cu * out[2]).sum()).backward()
    g2 = chain2.rolloutParameterAdjoint(det(tq), det(tdq), det(ttau), DT, r[3], r[4], gq_end=cq, integrator=integrator, components=cs2, feedback=fbd,
                                        gu_traj=cu)
    assert torch.equal(pi.grad.cuda(), g2[3])


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_without_parameters_it_is_rollout_with_feedback(mode):
    torch = pytest.importorskip("torch")
    from rosdyn_amd import Feedback, autograd
    integrator, hold = mode
    name = "ur10_like"
    chain = _chain(name)
    n, N, T = chain.getActiveJointsNumber(), 65, 3
    cs = _set(_specs(n), n)
    cq, cv, ct, cu = (torch.from_numpy(x).cuda() for x in _seeds(n, N, T, seed=15300))
    res = []
    for f in (autograd.closed_loop_rollout, lambda chain, q, dq, tau, dt, fb, **kw: autograd.rollout(chain, q, dq, tau, dt, feedback=fb, **kw)):
        a = _leaves(torch, name, n, N, T, 15300)
        fb = Feedback(a[3], a[5], a[6], a[4], hold=hold, tau_limit=a[7], command_trajectory=True)
        out = f(chain, a[0], a[1], a[2], DT, fb, integrator=integrator, trajectory=True, components=cs)
        assert len(out) == 5
        ((cq * out[0]).sum() + (cv * out[1]).sum() + (ct * out[3]).sum() + (cu * out[4]).sum()).backward()
        res.append((out, a))
    for x, y in zip(res[0][0], res[1][0]):
        assert torch.equal(x, y)
    for x, y in zip(res[0][1], res[1][1]):
        assert x.grad is not None and torch.equal(x.grad, y.grad)
    with pytest.raises(ValueError, match="needs feedback"):
        autograd.closed_loop_rollout(chain, res[0][1][0], res[0][1][1], res[0][1][2], DT, None)
