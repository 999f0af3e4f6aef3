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

Gradients with respect to the MODEL (output-error identification): both helpers take ``parameters`` -- a float64 tensor of shape
(10 chain.getJointsNumber(),), the inertial parameters in the order of ``Chain.getNominalParameters`` -- and ``component_parameters`` --
a float64 tensor of shape (components.columns,), in column order.  Either may live on any device.  The forward then runs on
``chain.withParameters(parameters)`` / ``components.withParameters(component_parameters)``: the values make a HOST ROUND TRIP (a
device-to-host copy and a new chain per call; a chain is a host object) -- small against a rollout, but a synchronisation.  The backward
returns dL/dparameters and dL/dcomponent_parameters on those tensors' devices, from ``Chain.getJointAccelerationParameterVjp`` (the sums)
and ``Chain.rolloutParameterAdjoint``: sums over the samples whose status is 1 -- a failed sample is NaN in its own state gradients and
adds NOTHING to the parameter gradients.  Without these arguments the two classes above are used, unchanged.

External link wrenches: both helpers take ``ext_wrenches`` (a tensor shaped as ``Chain.getJointAcceleration`` / ``Chain.rollout`` take
it, differentiable) and ``ext_link``.  They run through ``JointAccelerationExtFunction`` / ``RolloutExtFunction``, whose backward is
``Chain.getJointAccelerationVjp(ext_wrenches=)`` / ONE ``Chain.rolloutAdjoint(ext_wrenches=)`` call.  In ``rollout`` a wrench shaped like
one step's record is held over the horizon and its gradient is the sum over the steps; a leading ``T`` axis means one record per step.
Wrenches together with ``parameters`` / ``component_parameters`` raise ValueError: the parameter gradients with wrenches are the
follow-up (include/rdyn.h).

The closed loop: ``rollout`` takes ``feedback`` (a ``rosdyn_amd.Feedback``, as ``Chain.rollout`` takes it) and runs through
``RolloutFeedbackFunction``, whose backward is ONE ``Chain.rolloutAdjoint(feedback=)`` call -- the exact transpose of the loop, the PD
law and its clamp included.  Gradients flow to q0, Dq0, tau (now the feed-forward term) and to ``feedback.q_ref``, ``Dq_ref``, ``kp``,
``kd`` and ``tau_limit``, whichever require grad: shared gains and the limits get the sum of the per-sample rows, a reference held over
the horizon the sum over the steps.  With ``ext_wrenches`` the wrench gradient flows as above.  With ``feedback.command_trajectory`` the
command trajectory (one record per step: the command of the step's first evaluation) is returned last and is differentiable: a cost
on the control effort.  A clamped command has no slope: its gradient goes to ``tau_limit``.  ``parameters`` / ``component_parameters``
together with ``feedback`` raise ValueError in ``rollout``: the parameter gradients of the closed loop were its follow-up and are served by

    q_T, Dq_T, ... = closed_loop_rollout(chain, q0, Dq0, tau, dt, feedback, parameters=pi, component_parameters=cp)

(closed-loop output-error identification).  Without parameters it returns what ``rollout(feedback=)`` returns; with them it runs through
``RolloutFeedbackParametersFunction``: the model is built as above (``withParameters``, the host round trip), gradients flow to q0, Dq0,
tau, the law's tensors, ``parameters`` and ``component_parameters``, and the backward is ONE ``Chain.rolloutParameterAdjoint(feedback=)``
call (include/rdyn.h: rdyn_rollout_adjoint_feedback_parameters).  The law does not depend on the model: the parameter gradients are the
open loop's products, taken at the commands the closed loop applied.  External link wrenches are not among its arguments yet.
"""
import torch

__all__ = ["joint_acceleration", "rollout", "closed_loop_rollout", "RolloutFeedbackParametersFunction", "JointAccelerationFunction", "RolloutFunction", "JointAccelerationParametersFunction",
           "RolloutParametersFunction", "JointAccelerationExtFunction", "RolloutExtFunction", "RolloutFeedbackFunction"]


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


def _with_parameters(chain, components, parameters, component_parameters):
    """the chain and the component set the forward runs on"""
    if parameters is not None:
        if parameters.dtype != torch.float64 or parameters.dim() != 1:
            raise ValueError("parameters must be a float64 tensor of shape (10 * chain.getJointsNumber(),)")
        chain = chain.withParameters(parameters.detach().cpu().numpy())
    if component_parameters is not None:
        if components is None:
            raise ValueError("component_parameters need components")
        if component_parameters.dtype != torch.float64 or component_parameters.dim() != 1:
            raise ValueError("component_parameters must be a float64 tensor of shape (components.columns,)")
        components = components.withParameters(component_parameters.detach().cpu().tolist())
    return chain, components


def _parameter_grads(ctx, gpi, gcomp, first):
    """the last two entries of a backward's result"""
    need = ctx.needs_input_grad[first:first + 2]
    return (gpi.to(ctx.devices[0]) if need[0] and ctx.devices[0] is not None else None,
            gcomp.to(ctx.devices[1]) if need[1] and ctx.devices[1] is not None and gcomp is not None else None)


class JointAccelerationParametersFunction(torch.autograd.Function):
    """JointAccelerationFunction with the model among the inputs (parameters and component_parameters: each a tensor or None)"""

    @staticmethod
    def forward(ctx, chain, components, layout, q, Dq, tau, parameters, component_parameters):
        q, Dq, tau = q.detach().contiguous(), Dq.detach().contiguous(), tau.detach().contiguous()
        chain, components = _with_parameters(chain, components, parameters, component_parameters)
        ddq, _ = chain.getJointAcceleration(q, Dq, tau, layout=layout, components=components)
        ctx.chain, ctx.components, ctx.layout = chain, components, layout
        ctx.devices = tuple(t.device if t is not None else None for t in (parameters, component_parameters))
        ctx.save_for_backward(q, Dq, tau)
        return ddq

    @staticmethod
    def backward(ctx, g):
        q, Dq, tau = ctx.saved_tensors
        g = g.contiguous()
        grads = {}
        gpi = gcomp = None
        if any(ctx.needs_input_grad[6:8]):
            # (the parameter call returns tau_bar as well -- the same bits: the state product below is then asked for q and dq only)
            gpi, gcomp, grads["tau"] = ctx.chain.getJointAccelerationParameterVjp(q, Dq, tau, g, components=ctx.components, layout=ctx.layout,
                                                                                 reduce=True)[:3]
        names = tuple(k for k, need in zip(("q", "dq", "tau"), ctx.needs_input_grad[3:6]) if need and k not in grads)
        if names:
            res = ctx.chain.getJointAccelerationVjp(q, Dq, tau, g, layout=ctx.layout, want=names, components=ctx.components)
            grads.update(zip(names, res[1:]))
        if not ctx.needs_input_grad[5]:
            grads.pop("tau", None)
        return (None, None, None, grads.get("q"), grads.get("dq"), grads.get("tau")) + _parameter_grads(ctx, gpi, gcomp, 6)


class RolloutParametersFunction(torch.autograd.Function):
    """RolloutFunction with the model among the inputs; the backward is ONE Chain.rolloutParameterAdjoint call"""

    @staticmethod
    def forward(ctx, chain, components, layout, integrator, dt, n_steps, trajectory, q0, Dq0, tau, parameters, component_parameters):
        q0, Dq0, tau = q0.detach().contiguous(), Dq0.detach().contiguous(), tau.detach().contiguous()
        chain, components = _with_parameters(chain, components, parameters, component_parameters)
        q_end, dq_end, _, q_traj, dq_traj = chain.rollout(q0, Dq0, tau, dt, integrator=integrator, n_steps=n_steps, layout=layout,
                                                          trajectory_every=1, components=components)
        ctx.chain, ctx.components, ctx.layout, ctx.integrator, ctx.dt = chain, components, layout, integrator, dt
        ctx.n_steps, ctx.trajectory, ctx.sum_tau = q_traj.shape[0], trajectory, tau.dim() == 2
        ctx.devices = tuple(t.device if t is not None else None for t in (parameters, component_parameters))
        ctx.save_for_backward(q0, Dq0, tau, q_traj, dq_traj)
        if trajectory:
            return q_end, dq_end, q_traj.clone(), dq_traj.clone()  # (the saved records must not be written to by the caller)
        return q_end, dq_end

    @staticmethod
    def backward(ctx, gq_end, gdq_end, gq_traj=None, gdq_traj=None):
        q0, Dq0, tau, q_traj, dq_traj = ctx.saved_tensors
        c = lambda t: t.contiguous() if t is not None else None
        gq0, gdq0, gtau, gpi, gcomp, _ = ctx.chain.rolloutParameterAdjoint(q0, Dq0, tau, ctx.dt, q_traj, dq_traj, gq_end=c(gq_end),
                                                                           gDq_end=c(gdq_end), gq_traj=c(gq_traj), gDq_traj=c(gdq_traj),
                                                                           integrator=ctx.integrator, n_steps=ctx.n_steps, layout=ctx.layout,
                                                                           components=ctx.components, sum_tau=ctx.sum_tau)
        need = ctx.needs_input_grad[7:10]
        return ((None,) * 7 + (gq0 if need[0] else None, gdq0 if need[1] else None, gtau if need[2] else None)
                + _parameter_grads(ctx, gpi, gcomp, 10))


class JointAccelerationExtFunction(torch.autograd.Function):
    """JointAccelerationFunction with external link wrenches among the inputs"""

    @staticmethod
    def forward(ctx, chain, components, layout, ext_link, q, Dq, tau, ext_wrenches):
        q, Dq, tau, w = (t.detach().contiguous() for t in (q, Dq, tau, ext_wrenches))
        ddq, _ = chain.getJointAcceleration(q, Dq, tau, layout=layout, components=components, ext_wrenches=w, ext_link=ext_link)
        ctx.chain, ctx.components, ctx.layout, ctx.ext_link = chain, components, layout, ext_link
        ctx.save_for_backward(q, Dq, tau, w)
        return ddq

    @staticmethod
    def backward(ctx, g):
        q, Dq, tau, w = ctx.saved_tensors
        names = tuple(k for k, need in zip(("q", "dq", "tau", "ext"), ctx.needs_input_grad[4:8]) if need)
        if not names:
            return (None,) * 8
        res = ctx.chain.getJointAccelerationVjp(q, Dq, tau, g.contiguous(), layout=ctx.layout, want=names, components=ctx.components,
                                                ext_wrenches=w, ext_link=ctx.ext_link)
        grads = dict(zip(names, res[1:]))
        return None, None, None, None, grads.get("q"), grads.get("dq"), grads.get("tau"), grads.get("ext")


class RolloutExtFunction(torch.autograd.Function):
    """RolloutFunction with external link wrenches among the inputs; the backward is ONE Chain.rolloutAdjoint(ext_wrenches=) call"""

    @staticmethod
    def forward(ctx, chain, components, layout, integrator, dt, n_steps, trajectory, ext_link, q0, Dq0, tau, ext_wrenches):
        q0, Dq0, tau, w = (t.detach().contiguous() for t in (q0, Dq0, tau, ext_wrenches))
        q_end, dq_end, _, q_traj, dq_traj = chain.rollout(q0, Dq0, tau, dt, integrator=integrator, n_steps=n_steps, layout=layout,
                                                          trajectory_every=1, components=components, ext_wrenches=w, ext_link=ext_link)
        ctx.chain, ctx.components, ctx.layout, ctx.integrator, ctx.dt, ctx.ext_link = chain, components, layout, integrator, dt, ext_link
        ctx.n_steps, ctx.trajectory, ctx.sum_tau = q_traj.shape[0], trajectory, tau.dim() == 2
        ctx.sum_ext = w.dim() == (2 if ext_link is not None else (3 if layout == "sample" else 2))  # one record: held over the horizon
        ctx.save_for_backward(q0, Dq0, tau, q_traj, dq_traj, w)
        if trajectory:
            return q_end, dq_end, q_traj.clone(), dq_traj.clone()  # (the saved records must not be written to by the caller)
        return q_end, dq_end

    @staticmethod
    def backward(ctx, gq_end, gdq_end, gq_traj=None, gdq_traj=None):
        q0, Dq0, tau, q_traj, dq_traj, w = ctx.saved_tensors
        c = lambda t: t.contiguous() if t is not None else None
        res = ctx.chain.rolloutAdjoint(q0, Dq0, tau, ctx.dt, q_traj, dq_traj, gq_end=c(gq_end), gDq_end=c(gdq_end), gq_traj=c(gq_traj),
                                       gDq_traj=c(gdq_traj), integrator=ctx.integrator, n_steps=ctx.n_steps, layout=ctx.layout,
                                       components=ctx.components, sum_tau=ctx.sum_tau, ext_wrenches=w, ext_link=ctx.ext_link,
                                       want_ext=bool(ctx.needs_input_grad[11]), sum_ext=ctx.sum_ext)
        gq0, gdq0, gtau = res[:3]
        gext = None
        if ctx.needs_input_grad[11]:
            gext = res[4]
            if not ctx.sum_ext and gext.shape[0] < w.shape[0]:  # a sequence longer than the horizon: the unused records get 0
                gext = torch.cat([gext, gext.new_zeros((w.shape[0] - gext.shape[0],) + tuple(gext.shape[1:]))])
        need = ctx.needs_input_grad[8:11]
        return (None,) * 8 + (gq0 if need[0] else None, gdq0 if need[1] else None, gtau if need[2] else None, gext)


def _refuse_model_law(feedback):
    from .feedback import ModelFeedback
    if isinstance(feedback, ModelFeedback):
        raise NotImplementedError("rosdyn_amd.autograd does not differentiate a model-based law (rosdyn_amd.ModelFeedback) yet: its adjoint is "
                                  "the follow-up; Chain.rollout(feedback=) runs it forward")


class RolloutFeedbackFunction(torch.autograd.Function):
    """RolloutFunction around the closed loop: the law's references, gains and limits (and, optionally, external link wrenches) among the
    inputs, the command trajectory (optionally) among the outputs; the backward is ONE Chain.rolloutAdjoint(feedback=) call.  Dq_ref, kd,
    tau_limit and ext_wrenches may be None."""

    NAMES = ("q_ref", "Dq_ref", "kp", "kd", "tau_limit")

    @staticmethod
    def forward(ctx, chain, components, layout, integrator, dt, n_steps, trajectory, ext_link, hold, command, q0, Dq0, tau, q_ref, Dq_ref,
                kp, kd, tau_limit, ext_wrenches):
        from .feedback import Feedback
        det = lambda t: t.detach().contiguous() if t is not None else None
        q0, Dq0, tau, q_ref, Dq_ref, kp, kd, tau_limit, w = (det(t) for t in (q0, Dq0, tau, q_ref, Dq_ref, kp, kd, tau_limit, ext_wrenches))
        fb = Feedback(q_ref, kp, kd, Dq_ref, hold=hold, tau_limit=tau_limit, command_trajectory=command)
        res = chain.rollout(q0, Dq0, tau, dt, integrator=integrator, n_steps=n_steps, layout=layout, trajectory_every=1, components=components,
                            ext_wrenches=w, ext_link=ext_link, feedback=fb)
        q_end, dq_end, q_traj, dq_traj = res[0], res[1], res[3], res[4]
        ctx.chain, ctx.components, ctx.layout, ctx.integrator, ctx.dt, ctx.ext_link = chain, components, layout, integrator, dt, ext_link
        ctx.n_steps, ctx.trajectory, ctx.sum_tau, ctx.hold, ctx.command = q_traj.shape[0], trajectory, tau.dim() == 2, hold, command
        ctx.sum_ext = w is not None and w.dim() == (2 if ext_link is not None else (3 if layout == "sample" else 2))
        ctx.present = tuple(t is not None for t in (Dq_ref, kd, tau_limit, w))
        z = q0.new_empty((0,))
        ctx.save_for_backward(q0, Dq0, tau, q_traj, dq_traj, q_ref, kp, *(t if t is not None else z for t in (Dq_ref, kd, tau_limit, w)))
        out = (q_end, dq_end)
        if trajectory:
            out += (q_traj.clone(), dq_traj.clone())  # (the saved records must not be written to by the caller)
        if command:
            out += (res[5],)
        return out

    @staticmethod
    def backward(ctx, gq_end, gdq_end, *rest):
        from .feedback import Feedback
        q0, Dq0, tau, q_traj, dq_traj, q_ref, kp = ctx.saved_tensors[:7]
        Dq_ref, kd, tau_limit, w = (t if have else None for t, have in zip(ctx.saved_tensors[7:], ctx.present))
        c = lambda t: t.contiguous() if t is not None else None
        rest = list(rest)
        gq_traj, gdq_traj = (rest.pop(0), rest.pop(0)) if ctx.trajectory else (None, None)
        gu = rest.pop(0) if ctx.command else None
        need = dict(zip(RolloutFeedbackFunction.NAMES, ctx.needs_input_grad[13:18]))
        tensors = dict(zip(RolloutFeedbackFunction.NAMES, (q_ref, Dq_ref, kp, kd, tau_limit)))
        names = tuple(k for k in RolloutFeedbackFunction.NAMES if need[k] and tensors[k] is not None)
        want_ext = w is not None and bool(ctx.needs_input_grad[18])
        fb = Feedback(q_ref, kp, kd, Dq_ref, hold=ctx.hold, tau_limit=tau_limit)
        res = ctx.chain.rolloutAdjoint(q0, Dq0, tau, ctx.dt, q_traj, dq_traj, gq_end=c(gq_end), gDq_end=c(gdq_end), gq_traj=c(gq_traj),
                                       gDq_traj=c(gdq_traj), integrator=ctx.integrator, n_steps=ctx.n_steps, layout=ctx.layout,
                                       components=ctx.components, sum_tau=ctx.sum_tau, ext_wrenches=w, ext_link=ctx.ext_link if w is not None else None,
                                       want_ext=want_ext, sum_ext=ctx.sum_ext if w is not None else False, feedback=fb, want_feedback=names,
                                       gu_traj=c(gu))
        gq0, gdq0, gtau = res[:3]

        def padded(g, like):  # a sequence longer than the horizon: the unused records get 0
            if g.dim() == like.dim() and g.shape[0] < like.shape[0]:
                g = torch.cat([g, g.new_zeros((like.shape[0] - g.shape[0],) + tuple(g.shape[1:]))])
            return g

        gext = None
        at = 4
        if want_ext:
            gext = res[at] if ctx.sum_ext else padded(res[at], w)
            at += 1
        grads = dict(zip(names, res[at:]))
        for k in ("q_ref", "Dq_ref"):
            if k in grads:
                grads[k] = padded(grads[k], tensors[k])
        for k in ("kp", "kd", "tau_limit"):
            if k in grads and tensors[k].dim() == 1:  # shared by the samples: the sum of their rows
                grads[k] = grads[k].sum(dim=0 if ctx.layout == "sample" else 1)
        n3 = ctx.needs_input_grad[10:13]
        return ((None,) * 10 + (gq0 if n3[0] else None, gdq0 if n3[1] else None, gtau if n3[2] else None)
                + tuple(grads.get(k) for k in RolloutFeedbackFunction.NAMES) + (gext,))


class RolloutFeedbackParametersFunction(torch.autograd.Function):
    """RolloutFeedbackFunction (without wrenches) with the model among the inputs; the backward is ONE
    Chain.rolloutParameterAdjoint(feedback=) call.  Dq_ref, kd, tau_limit, parameters and component_parameters may be None."""

    @staticmethod
    def forward(ctx, chain, components, layout, integrator, dt, n_steps, trajectory, hold, command, q0, Dq0, tau, q_ref, Dq_ref, kp, kd,
                tau_limit, parameters, component_parameters):
        from .feedback import Feedback
        det = lambda t: t.detach().contiguous() if t is not None else None
        q0, Dq0, tau, q_ref, Dq_ref, kp, kd, tau_limit = (det(t) for t in (q0, Dq0, tau, q_ref, Dq_ref, kp, kd, tau_limit))
        chain, components = _with_parameters(chain, components, parameters, component_parameters)
        fb = Feedback(q_ref, kp, kd, Dq_ref, hold=hold, tau_limit=tau_limit, command_trajectory=command)
        res = chain.rollout(q0, Dq0, tau, dt, integrator=integrator, n_steps=n_steps, layout=layout, trajectory_every=1, components=components,
                            feedback=fb)
        q_end, dq_end, q_traj, dq_traj = res[0], res[1], res[3], res[4]
        ctx.chain, ctx.components, ctx.layout, ctx.integrator, ctx.dt = chain, components, layout, integrator, dt
        ctx.n_steps, ctx.trajectory, ctx.sum_tau, ctx.hold, ctx.command = q_traj.shape[0], trajectory, tau.dim() == 2, hold, command
        ctx.present = tuple(t is not None for t in (Dq_ref, kd, tau_limit))
        ctx.devices = tuple(t.device if t is not None else None for t in (parameters, component_parameters))
        z = q0.new_empty((0,))
        ctx.save_for_backward(q0, Dq0, tau, q_traj, dq_traj, q_ref, kp, *(t if t is not None else z for t in (Dq_ref, kd, tau_limit)))
        out = (q_end, dq_end)
        if trajectory:
            out += (q_traj.clone(), dq_traj.clone())  # (the saved records must not be written to by the caller)
        if command:
            out += (res[5],)
        return out

    @staticmethod
    def backward(ctx, gq_end, gdq_end, *rest):
        from .feedback import Feedback
        q0, Dq0, tau, q_traj, dq_traj, q_ref, kp = ctx.saved_tensors[:7]
        Dq_ref, kd, tau_limit = (t if have else None for t, have in zip(ctx.saved_tensors[7:], ctx.present))
        c = lambda t: t.contiguous() if t is not None else None
        rest = list(rest)
        gq_traj, gdq_traj = (rest.pop(0), rest.pop(0)) if ctx.trajectory else (None, None)
        gu = rest.pop(0) if ctx.command else None
        NAMES = RolloutFeedbackFunction.NAMES
        need = dict(zip(NAMES, ctx.needs_input_grad[12:17]))
        tensors = dict(zip(NAMES, (q_ref, Dq_ref, kp, kd, tau_limit)))
        names = tuple(k for k in NAMES if need[k] and tensors[k] is not None)
        fb = Feedback(q_ref, kp, kd, Dq_ref, hold=ctx.hold, tau_limit=tau_limit)
        res = ctx.chain.rolloutParameterAdjoint(q0, Dq0, tau, ctx.dt, q_traj, dq_traj, gq_end=c(gq_end), gDq_end=c(gdq_end), gq_traj=c(gq_traj),
                                                gDq_traj=c(gdq_traj), integrator=ctx.integrator, n_steps=ctx.n_steps, layout=ctx.layout,
                                                components=ctx.components, sum_tau=ctx.sum_tau, feedback=fb, want_feedback=names,
                                                gu_traj=c(gu))
        gq0, gdq0, gtau, gpi, gcomp = res[:5]
        grads = dict(zip(names, res[6:]))
        for k in ("q_ref", "Dq_ref"):  # a sequence longer than the horizon: the unused records get 0
            if k in grads and grads[k].dim() == tensors[k].dim() and grads[k].shape[0] < tensors[k].shape[0]:
                g = grads[k]
                grads[k] = torch.cat([g, g.new_zeros((tensors[k].shape[0] - g.shape[0],) + tuple(g.shape[1:]))])
        for k in ("kp", "kd", "tau_limit"):
            if k in grads and tensors[k].dim() == 1:  # shared by the samples: the sum of their rows
                grads[k] = grads[k].sum(dim=0 if ctx.layout == "sample" else 1)
        n3 = ctx.needs_input_grad[9:12]
        return ((None,) * 9 + (gq0 if n3[0] else None, gdq0 if n3[1] else None, gtau if n3[2] else None)
                + tuple(grads.get(k) for k in NAMES) + _parameter_grads(ctx, gpi, gcomp, 17))


def _no_parameters_with_wrenches(parameters, component_parameters):
    if parameters is not None or component_parameters is not None:
        raise ValueError("ext_wrenches together with parameters / component_parameters is not served yet: the parameter gradients with "
                         "external wrenches are the follow-up")


def joint_acceleration(chain, q, Dq, tau, components=None, layout="sample", parameters=None, component_parameters=None, ext_wrenches=None,
                       ext_link=None):
    """Differentiable ``Chain.getJointAcceleration``: DDq = FD_c(q, Dq, tau), shaped like q.  Gradients flow to q, Dq and tau through
    ``Chain.getJointAccelerationVjp``.  A sample with status -1 is NaN in DDq and in its gradients; nothing is raised.
    parameters / component_parameters (the module docstring): the model to evaluate, differentiable as well.
    ext_wrenches, ext_link (the module docstring): external link wrenches as ``Chain.getJointAcceleration`` takes them, differentiable."""
    if ext_wrenches is not None:
        _no_parameters_with_wrenches(parameters, component_parameters)
        return JointAccelerationExtFunction.apply(chain, components, layout, ext_link, q, Dq, tau, ext_wrenches)
    if parameters is None and component_parameters is None:
        return JointAccelerationFunction.apply(chain, components, layout, q, Dq, tau)
    return JointAccelerationParametersFunction.apply(chain, components, layout, q, Dq, tau, parameters, component_parameters)


def rollout(chain, q0, Dq0, tau, dt, integrator="rk4", n_steps=None, trajectory=False, components=None, layout="sample", parameters=None,
            component_parameters=None, ext_wrenches=None, ext_link=None, feedback=None):
    """Differentiable ``Chain.rollout``: returns (q_end, Dq_end), and with trajectory=True also (q_traj, Dq_traj) with one record per
    step (record k = the state after step k + 1).  tau: (T, N, n) / (T, n, N), one torque per step, or shaped like q0 with an explicit
    n_steps (held over the horizon: its gradient is the sum over the steps).  Gradients flow to q0, Dq0 and tau from the end state and
    from every trajectory record; the backward is one ``Chain.rolloutAdjoint`` call over the records the forward saved.
    A sample whose rollout reports status -1 has NaN states from the failing step on and NaN gradients; nothing is raised.
    parameters / component_parameters (the module docstring): the model to simulate, differentiable as well -- the backward is then one
    ``Chain.rolloutParameterAdjoint`` call (chains with at most 10 input joints).
    ext_wrenches, ext_link (the module docstring): external link wrenches as ``Chain.rollout`` takes them, differentiable: one step's
    record is held over the horizon (its gradient is the sum over the steps), a leading T axis is one record per step.
    feedback (the module docstring): a ``rosdyn_amd.Feedback``, the closed loop; tau is its feed-forward term and the law's tensors are
    differentiable.  With ``feedback.command_trajectory`` the command trajectory is appended to the returned tuple.  A
    ``rosdyn_amd.ModelFeedback`` raises NotImplementedError: the adjoint of the model-based laws is not served yet."""
    _refuse_model_law(feedback)
    if n_steps is None:
        if tau.dim() != 3:
            raise ValueError("torques shaped like q0 need an explicit n_steps")
        n_steps = tau.shape[0]
    if feedback is not None:
        if parameters is not None or component_parameters is not None:
            raise ValueError("feedback together with parameters / component_parameters is not served by rollout: the parameter gradients "
                             "of the closed loop, its follow-up, come from closed_loop_rollout")
        return RolloutFeedbackFunction.apply(chain, components, layout, integrator, float(dt), int(n_steps), bool(trajectory), ext_link,
                                             bool(feedback.hold), bool(feedback.command_trajectory), q0, Dq0, tau, feedback.q_ref,
                                             feedback.Dq_ref, feedback.kp, feedback.kd, feedback.tau_limit, ext_wrenches)
    if ext_wrenches is not None:
        _no_parameters_with_wrenches(parameters, component_parameters)
        return RolloutExtFunction.apply(chain, components, layout, integrator, float(dt), int(n_steps), bool(trajectory), ext_link, q0, Dq0,
                                        tau, ext_wrenches)
    if parameters is None and component_parameters is None:
        return RolloutFunction.apply(chain, components, layout, integrator, float(dt), int(n_steps), bool(trajectory), q0, Dq0, tau)
    return RolloutParametersFunction.apply(chain, components, layout, integrator, float(dt), int(n_steps), bool(trajectory), q0, Dq0, tau,
                                           parameters, component_parameters)


def closed_loop_rollout(chain, q0, Dq0, tau, dt, feedback, integrator="rk4", n_steps=None, trajectory=False, components=None, layout="sample",
                        parameters=None, component_parameters=None):
    """Differentiable ``Chain.rollout(feedback=)`` with the model among the inputs (the module docstring): what closed-loop output-error
    identification descends through.  feedback: a ``rosdyn_amd.Feedback``; tau is its feed-forward term.  Returns (q_end, Dq_end), with
    trajectory=True also (q_traj, Dq_traj), and with ``feedback.command_trajectory`` the command trajectory last.
    Without parameters and component_parameters it returns what ``rollout(feedback=)`` returns.  With either, the closed loop runs on
    ``chain.withParameters(parameters)`` / ``components.withParameters(component_parameters)`` and gradients flow to q0, Dq0, tau, the
    law's tensors, parameters and component_parameters; the backward is one ``Chain.rolloutParameterAdjoint(feedback=)`` call (chains
    that call serves: at most 10 input joints).  A failed sample is NaN in its own gradients and adds nothing to the parameter gradients."""
    if feedback is None:
        raise ValueError("closed_loop_rollout needs feedback (rollout serves the open loop)")
    _refuse_model_law(feedback)
    if parameters is None and component_parameters is None:
        return rollout(chain, q0, Dq0, tau, dt, integrator=integrator, n_steps=n_steps, trajectory=trajectory, components=components,
                       layout=layout, feedback=feedback)
    if n_steps is None:
        if tau.dim() != 3:
            raise ValueError("torques shaped like q0 need an explicit n_steps")
        n_steps = tau.shape[0]
    return RolloutFeedbackParametersFunction.apply(chain, components, layout, integrator, float(dt), int(n_steps), bool(trajectory),
                                                   bool(feedback.hold), bool(feedback.command_trajectory), q0, Dq0, tau, feedback.q_ref,
                                                   feedback.Dq_ref, feedback.kp, feedback.kd, feedback.tau_limit, parameters,
                                                   component_parameters)
