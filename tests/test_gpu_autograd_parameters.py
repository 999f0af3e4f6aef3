"""GPU tests of rosdyn_amd.autograd with the model among the inputs: loss.backward() through joint_acceleration / rollout fills the gradients
of `parameters` and `component_parameters` with the bits of Chain.getJointAccelerationParameterVjp (the sums) / Chain.rolloutParameterAdjoint,
leaves the gradients of the state and the torques those of the existing path, and changes nothing where the new arguments are not used."""
import numpy as np
import pytest

from _arrays import INTEGRATORS, _adjoint_inputs as _inputs, _dev, _dev_seq
from _chains import _cpair
from _components import _set, _specs

pytestmark = pytest.mark.gpu


def _model(torch, chain, n, device):
    """(components, pi, p): the chain's parameters moved by a few percent, as leaves on `device`"""
    cs = _set(_specs(n), n)
    rng = np.random.default_rng(17)
    pi0 = chain.getNominalParameters()
    pi = torch.tensor(pi0 * (1.0 + 0.05 * rng.uniform(-1, 1, pi0.shape)), dtype=torch.float64, device=device, requires_grad=True)
    p0 = np.array(cs.getNominalParameters())
    p = torch.tensor(p0 * (1.0 + 0.05 * rng.uniform(-1, 1, p0.shape)), dtype=torch.float64, device=device, requires_grad=True)
    return cs, pi, p


@pytest.mark.parametrize("device", ["cpu", "cuda"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", ["ur10_like", "ur10_public_long"])
def test_backward_through_a_rollout_fills_the_parameter_gradients(name, integrator, device):
    torch = pytest.importorskip("torch")
    from rosdyn_amd import autograd
    chain, _ = _cpair(name, oracle=False)
    n, N, T, dt = chain.getActiveJointsNumber(), 65, 3, 1e-3
    cs, pi, p = _model(torch, chain, n, device)
    q0, dq0, tau = _inputs(name, n, N, T, seed=9100)
    tq, tdq, ttau = (_dev(torch, q0, "sample").requires_grad_(), _dev(torch, dq0, "sample").requires_grad_(),
                     _dev_seq(torch, tau, "sample").requires_grad_())
    wq, wv = (torch.rand((N, n), dtype=torch.float64, device="cuda") for _ in range(2))
    q_end, dq_end = autograd.rollout(chain, tq, tdq, ttau, dt, integrator=integrator, components=cs, parameters=pi, component_parameters=p)
    ((q_end * wq).sum() + (dq_end * wv).sum()).backward()
    assert pi.grad.device == pi.device and p.grad.device == p.device and pi.grad.shape == pi.shape and p.grad.shape == p.shape
    # the direct calls on the same model
    chain2, cs2 = chain.withParameters(pi.detach().cpu().numpy()), cs.withParameters(p.detach().cpu().tolist())
    r = chain2.rollout(tq.detach(), tdq.detach(), ttau.detach(), dt, integrator=integrator, trajectory_every=1, components=cs2)
    assert torch.equal(q_end, r[0]) and torch.equal(dq_end, r[1]) and bool((r[2] == 1).all())
    g = chain2.rolloutParameterAdjoint(tq.detach(), tdq.detach(), ttau.detach(), dt, r[3], r[4], gq_end=wq, gDq_end=wv, integrator=integrator,
                                       components=cs2)
    assert torch.equal(pi.grad.cuda(), g[3]) and torch.equal(p.grad.cuda(), g[4]) and bool(g[3].abs().sum() > 0) and bool(g[4].abs().sum() > 0)
    # the state and torque gradients: the existing path on that model, bit for bit
    q2, dq2, tau2 = (t.detach().clone().requires_grad_() for t in (tq, tdq, ttau))
    e = autograd.rollout(chain2, q2, dq2, tau2, dt, integrator=integrator, components=cs2)
    ((e[0] * wq).sum() + (e[1] * wv).sum()).backward()
    assert torch.equal(tq.grad, q2.grad) and torch.equal(tdq.grad, dq2.grad) and torch.equal(ttau.grad, tau2.grad)
    # one of the two alone, and the trajectory records as outputs
    pi.grad = None
    out = autograd.rollout(chain, tq.detach(), tdq.detach(), ttau.detach(), dt, integrator=integrator, components=cs2, parameters=pi, trajectory=True)
    (out[2] * wq).sum().backward()
    g2 = chain2.rolloutParameterAdjoint(tq.detach(), tdq.detach(), ttau.detach(), dt, r[3], r[4], gq_traj=wq.expand(T, N, n).contiguous(),
                                        integrator=integrator, components=cs2)
    assert torch.equal(pi.grad.cuda(), g2[3])


@pytest.mark.parametrize("layout", ["sample", "element"])
@pytest.mark.parametrize("name", ["ur10_like", "ur10_public_long"])
def test_backward_through_the_forward_dynamics_fills_the_parameter_gradients(name, layout):
    torch = pytest.importorskip("torch")
    from rosdyn_amd import autograd
    chain, _ = _cpair(name, oracle=False)
    n, N = chain.getActiveJointsNumber(), 130
    cs, pi, p = _model(torch, chain, n, "cuda")
    q0, dq0, tau = _inputs(name, n, N, 1, seed=9300)
    tq, tdq, ttau = (_dev(torch, x, layout).requires_grad_() for x in (q0, dq0, tau[0]))
    w = torch.rand(tq.shape, dtype=torch.float64, device="cuda")
    ddq = autograd.joint_acceleration(chain, tq, tdq, ttau, components=cs, layout=layout, parameters=pi, component_parameters=p)
    (ddq * w).sum().backward()
    chain2, cs2 = chain.withParameters(pi.detach().cpu().numpy()), cs.withParameters(p.detach().cpu().tolist())
    want = chain2.getJointAccelerationParameterVjp(tq.detach(), tdq.detach(), ttau.detach(), w, components=cs2, layout=layout, reduce=True)
    assert torch.equal(pi.grad, want[0]) and torch.equal(p.grad, want[1]) and torch.equal(ddq, want[3]) and bool(want[0].abs().sum() > 0)
    q2, dq2, tau2 = (t.detach().clone().requires_grad_() for t in (tq, tdq, ttau))
    (autograd.joint_acceleration(chain2, q2, dq2, tau2, components=cs2, layout=layout) * w).sum().backward()
    assert torch.equal(tq.grad, q2.grad) and torch.equal(tdq.grad, dq2.grad) and torch.equal(ttau.grad, tau2.grad)


def test_without_the_new_arguments_nothing_changes():
    torch = pytest.importorskip("torch")
    from rosdyn_amd import autograd
    chain, _ = _cpair("ur10_like", oracle=False)
    n, N, T, dt = chain.getActiveJointsNumber(), 65, 3, 1e-3
    cs = _set(_specs(n), n)
    q0, dq0, tau = _inputs("ur10_like", n, N, T, seed=9500)
    res = []
    for use_helper in (True, False):
        tq, tdq, ttau = (_dev(torch, q0, "sample").requires_grad_(), _dev(torch, dq0, "sample").requires_grad_(),
                         _dev_seq(torch, tau, "sample").requires_grad_())
        if use_helper:
            e = autograd.rollout(chain, tq, tdq, ttau, dt, components=cs)
            a = autograd.joint_acceleration(chain, tq, tdq, ttau[0], components=cs)
        else:
            e = autograd.RolloutFunction.apply(chain, cs, "sample", "rk4", dt, T, False, tq, tdq, ttau)
            a = autograd.JointAccelerationFunction.apply(chain, cs, "sample", tq, tdq, ttau[0])
        (e[0].sum() + e[1].sum() + a.sum()).backward()
        res.append((e[0], e[1], a, tq.grad, tdq.grad, ttau.grad))
    assert all(torch.equal(x, y) for x, y in zip(*res))
