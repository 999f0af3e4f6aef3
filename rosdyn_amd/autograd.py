"""torch.autograd through the forward dynamics and through rollouts.

Two ``torch.autograd.Function`` wrappers over the reverse-mode calls of the C-ABI (include/rdyn.h: rdyn_forward_dynamics_vjp,
rdyn_rollout_adjoint) and the thin helpers that users call:

    ddq = joint_acceleration(chain, q, Dq, tau)                        # differentiable in q, Dq, tau
    q_T, Dq_T = rollout(chain, q0, Dq0, tau, dt, integrator="rk4")      # differentiable in q0, Dq0, tau
    q_T, Dq_T, q_traj, Dq_traj = rollout(..., trajectory=True)          # ... through every record as well

The backward of ``rollout`` is ONE ``Chain.rolloutAdjoint`` call: the exact transpose of the discrete integrator (both integrators),
not a differentiation of the continuous dynamics.  There is no eager-PyTorch path: forward and backward are the library's kernels.

Failed samples: a sample whose status is -1 (the inertia matrix is not positive definite, or a value is not finite) has NaN outputs in
the forward call and yields NaN gradients for that sample -- and only for it.  Nothing is raised, and the status words are not returned:
call ``Chain.getJointAcceleration`` / ``Chain.rollout`` directly where they are needed.
Component kinks: friction components are piecewise linear; exactly at a kink the gradient is the outer one-sided slope.
"""
import torch

__all__ = ["joint_acceleration", "rollout", "JointAccelerationFunction", "RolloutFunction"]


class JointAccelerationFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, chain, components, layout, q, Dq, tau):
        q, Dq, tau = q.detach().contiguous(), Dq.detach().contiguous(), tau.detach().contiguous()
        ddq, _ = chain.getJointAcceleration(q, Dq, tau, layout=layout, components=components)
        ctx.chain, ctx.components, ctx.layout = chain, components, layout
        ctx.save_for_backward(q, Dq, tau)
        return ddq

    @staticmethod
    def backward(ctx, g):
        q, Dq, tau = ctx.saved_tensors
        names = tuple(k for k, need in zip(("q", "dq", "tau"), ctx.needs_input_grad[3:6]) if need)
        if not names:
            return (None,) * 6
        res = ctx.chain.getJointAccelerationVjp(q, Dq, tau, g.contiguous(), layout=ctx.layout, want=names, components=ctx.components)
        grads = dict(zip(names, res[1:]))
        return None, None, None, grads.get("q"), grads.get("dq"), grads.get("tau")


class RolloutFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, chain, components, layout, integrator, dt, n_steps, trajectory, q0, Dq0, tau):
        q0, Dq0, tau = q0.detach().contiguous(), Dq0.detach().contiguous(), tau.detach().contiguous()
        q_end, dq_end, _, q_traj, dq_traj = chain.rollout(q0, Dq0, tau, dt, integrator=integrator, n_steps=n_steps, layout=layout,
                                                          trajectory_every=1, components=components)
        ctx.chain, ctx.components, ctx.layout, ctx.integrator, ctx.dt = chain, components, layout, integrator, dt
        ctx.n_steps, ctx.trajectory, ctx.sum_tau = q_traj.shape[0], trajectory, tau.dim() == 2
        ctx.save_for_backward(q0, Dq0, tau, q_traj, dq_traj)
        if trajectory:
            return q_end, dq_end, q_traj.clone(), dq_traj.clone()  # (the saved records must not be written to by the caller)
        return q_end, dq_end

    @staticmethod
    def backward(ctx, gq_end, gdq_end, gq_traj=None, gdq_traj=None):
        q0, Dq0, tau, q_traj, dq_traj = ctx.saved_tensors
        c = lambda t: t.contiguous() if t is not None else None
        gq0, gdq0, gtau, _ = ctx.chain.rolloutAdjoint(q0, Dq0, tau, ctx.dt, q_traj, dq_traj, gq_end=c(gq_end), gDq_end=c(gdq_end),
                                                      gq_traj=c(gq_traj), gDq_traj=c(gdq_traj), integrator=ctx.integrator,
                                                      n_steps=ctx.n_steps, layout=ctx.layout, components=ctx.components,
                                                      sum_tau=ctx.sum_tau)
        need = ctx.needs_input_grad[7:10]
        return (None,) * 7 + (gq0 if need[0] else None, gdq0 if need[1] else None, gtau if need[2] else None)


def joint_acceleration(chain, q, Dq, tau, components=None, layout="sample"):
    """Differentiable ``Chain.getJointAcceleration``: DDq = FD_c(q, Dq, tau), shaped like q.  Gradients flow to q, Dq and tau through
    ``Chain.getJointAccelerationVjp``.  A sample with status -1 is NaN in DDq and in its gradients; nothing is raised."""
    return JointAccelerationFunction.apply(chain, components, layout, q, Dq, tau)


def rollout(chain, q0, Dq0, tau, dt, integrator="rk4", n_steps=None, trajectory=False, components=None, layout="sample"):
    """Differentiable ``Chain.rollout``: returns (q_end, Dq_end), and with trajectory=True also (q_traj, Dq_traj) with one record per
    step (record k = the state after step k + 1).  tau: (T, N, n) / (T, n, N), one torque per step, or shaped like q0 with an explicit
    n_steps (held over the horizon: its gradient is the sum over the steps).  Gradients flow to q0, Dq0 and tau from the end state and
    from every trajectory record; the backward is one ``Chain.rolloutAdjoint`` call over the records the forward saved.
    A sample whose rollout reports status -1 has NaN states from the failing step on and NaN gradients; nothing is raised."""
    if n_steps is None:
        if tau.dim() != 3:
            raise ValueError("torques shaped like q0 need an explicit n_steps")
        n_steps = tau.shape[0]
    return RolloutFunction.apply(chain, components, layout, integrator, float(dt), int(n_steps), bool(trajectory), q0, Dq0, tau)
