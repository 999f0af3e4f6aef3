"""GPU tests of rosdyn_amd.autograd: torch.autograd through Chain.getJointAcceleration and Chain.rollout.

torch.autograd.gradcheck at its default tolerances (eps 1e-6, atol 1e-5, rtol 1e-3) compares the backward of the wrappers --
Chain.getJointAccelerationVjp, one Chain.rolloutAdjoint call -- with central differences of their own forward calls.  Components are
piecewise linear in Dq: they are included only where every |Dq| of the horizon keeps at least 0.05 from the kinks +-min_velocity,
+-max_velocity, asserted on the trajectory."""
import numpy as np
import pytest

from test_gpu_forward_dynamics import _chain
from test_gpu_rollout import INTEGRATORS, TAU_SCALE

pytestmark = pytest.mark.gpu
N, T, DT = 3, 4, 1e-2
FRICTION1, SPRING = 0, 2
MIN_VELOCITY, MAX_VELOCITY = 0.05, 1000.0


def _leaves(torch, name, n, steps=None, seed=8100, dq_offset=0.0):
    from rosdyn_amd.samples import uniform_pm1
    q = uniform_pm1(seed, (N, n))
    dq = uniform_pm1(seed + 1, (N, n)) + dq_offset
    tau = TAU_SCALE[name] * uniform_pm1(seed + 2, (N, n) if steps is None else (steps, N, n))
    return tuple(torch.from_numpy(x).cuda().requires_grad_(True) for x in (q, dq, tau))


def _components(n):
    """friction on the first two joints (band +-0.05, saturation far away), a spring on joint 0"""
    from rosdyn_amd.components import ComponentSet
    return ComponentSet([dict(type=FRICTION1, joint=0, min_velocity=MIN_VELOCITY, max_velocity=MAX_VELOCITY, parameters=[0.3, 0.2, 0.0]),
                         dict(type=FRICTION1, joint=1, min_velocity=MIN_VELOCITY, max_velocity=MAX_VELOCITY, parameters=[0.1, 0.05, 0.0]),
                         dict(type=SPRING, joint=0, min_velocity=0.0, max_velocity=0.0, parameters=[2.0, -0.1, 0.0])], n)


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
