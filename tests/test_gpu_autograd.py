"""GPU tests of rosdyn_amd.autograd: torch.autograd through Chain.getJointAcceleration and Chain.rollout.

torch.autograd.gradcheck at its default tolerances (eps 1e-6, atol 1e-5, rtol 1e-3) compares the backward of the wrappers --
Chain.getJointAccelerationVjp, one Chain.rolloutAdjoint call -- with central differences of their own forward calls.  Components are
piecewise linear in Dq: they are included only where every |Dq| of the horizon keeps at least 0.05 from the kinks +-min_velocity,
+-max_velocity, asserted on the trajectory."""
import numpy as np
import pytest

from _arrays import AUTOGRAD_DT as DT, AUTOGRAD_T as T, INTEGRATORS, _leaves
from _chains import _chain
from _components import AUTOGRAD_MAX_VELOCITY as MAX_VELOCITY, AUTOGRAD_MIN_VELOCITY as MIN_VELOCITY, _autograd_components as _components

pytestmark = pytest.mark.gpu


def _away_from_the_kinks(dq):
    a = np.abs(dq[..., [0, 1]])
    return bool((np.abs(a - MIN_VELOCITY) >= 0.05).all() and (np.abs(a - MAX_VELOCITY) >= 0.05).all())


@pytest.mark.parametrize("with_components", [False, True], ids=["plain", "components"])
@pytest.mark.parametrize("name", ["planar_2r", "ur10_like"])
def test_gradcheck_joint_acceleration(name, with_components):
    torch = pytest.importorskip("torch")
    from rosdyn_amd import autograd
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    cs = _components(n) if with_components else None
    q, dq, tau = _leaves(torch, name, n, dq_offset=3.0 if with_components else 0.0)
    if with_components:
        assert _away_from_the_kinks(dq.detach().cpu().numpy())
    assert torch.autograd.gradcheck(lambda a, b, c: autograd.joint_acceleration(chain, a, b, c, components=cs), (q, dq, tau))


@pytest.mark.parametrize("trajectory", [False, True], ids=["end_state", "trajectory"])
@pytest.mark.parametrize("with_components", [False, True], ids=["plain", "components"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", ["planar_2r", "ur10_like"])
def test_gradcheck_rollout(name, integrator, with_components, trajectory):
    torch = pytest.importorskip("torch")
    from rosdyn_amd import autograd
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    cs = _components(n) if with_components else None
    q0, dq0, tau = _leaves(torch, name, n, steps=T, seed=8200, dq_offset=3.0 if with_components else 0.0)
    if with_components:
        # the whole horizon, central-difference steps of 1e-6 included, stays 0.05 away from the kinks
        r = chain.rollout(q0.detach(), dq0.detach(), tau.detach(), DT, integrator=integrator, trajectory_every=1, components=cs)
        assert bool((r[2] == 1).all())
        assert _away_from_the_kinks(dq0.detach().cpu().numpy()) and _away_from_the_kinks(r[4].cpu().numpy())
    fn = lambda a, b, c: autograd.rollout(chain, a, b, c, DT, integrator=integrator, trajectory=trajectory, components=cs)
    assert len(fn(q0, dq0, tau)) == (4 if trajectory else 2)
    assert torch.autograd.gradcheck(fn, (q0, dq0, tau))


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_backward_populates_the_torque_gradient_with_the_adjoint_call_own_bits(integrator):
    torch = pytest.importorskip("torch")
    from rosdyn_amd import autograd
    name = "ur10_like"
    chain = _chain(name)
    n = chain.getActiveJointsNumber()
    q0, dq0, tau = _leaves(torch, name, n, steps=T, seed=8300)
    q_end, dq_end, q_traj, dq_traj = autograd.rollout(chain, q0, dq0, tau, DT, integrator=integrator, trajectory=True)
    cq, cv, rq = torch.rand_like(q_end), torch.rand_like(dq_end), torch.rand_like(q_traj)
    loss = (cq * q_end).sum() + (cv * dq_end).sum() + (rq * q_traj).sum()
    loss.backward()
    r = chain.rollout(q0.detach(), dq0.detach(), tau.detach(), DT, integrator=integrator, trajectory_every=1)
    assert torch.equal(r[0], q_end.detach()) and torch.equal(r[3], q_traj.detach())
    g = chain.rolloutAdjoint(q0.detach(), dq0.detach(), tau.detach(), DT, r[3], r[4], gq_end=cq, gDq_end=cv, gq_traj=rq,
                             gDq_traj=torch.zeros_like(rq), integrator=integrator)
    assert bool((g[3] == 1).all())
    assert torch.equal(tau.grad, g[2]) and torch.equal(q0.grad, g[0]) and torch.equal(dq0.grad, g[1])
    assert bool(tau.grad.abs().sum() > 0)
    # torques held over the horizon: the gradient is the adjoint call's sum over the steps
    q0b, dq0b, held = _leaves(torch, name, n, seed=8400)
    q_end, dq_end = autograd.rollout(chain, q0b, dq0b, held, DT, integrator=integrator, n_steps=T)
    ((cq * q_end).sum() + (cv * dq_end).sum()).backward()
    r = chain.rollout(q0b.detach(), dq0b.detach(), held.detach(), DT, integrator=integrator, n_steps=T, trajectory_every=1)
    g = chain.rolloutAdjoint(q0b.detach(), dq0b.detach(), held.detach(), DT, r[3], r[4], gq_end=cq, gDq_end=cv, integrator=integrator, n_steps=T,
                             sum_tau=True)
    assert held.grad.shape == held.shape and torch.equal(held.grad, g[2])


def test_a_failed_sample_yields_nan_gradients_for_that_sample_only():
    torch = pytest.importorskip("torch")
    from rosdyn_amd import autograd
    chain = _chain("ur10_like")
    n = chain.getActiveJointsNumber()
    q, dq, tau = _leaves(torch, "ur10_like", n, seed=8500)
    with torch.no_grad():
        q[1, 2] = float("nan")
    ddq = autograd.joint_acceleration(chain, q, dq, tau)
    assert bool(torch.isnan(ddq[1]).all()) and bool(torch.isfinite(ddq[[0, 2]]).all())
    torch.nan_to_num(ddq, nan=0.0).sum().backward()   # (a finite loss: the NaN comes from the backward call itself)
    for t in (q, dq, tau):
        assert bool(torch.isnan(t.grad[1]).all()) and bool(torch.isfinite(t.grad[[0, 2]]).all())
