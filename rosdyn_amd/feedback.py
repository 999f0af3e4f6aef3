"""The feedback laws of a closed-loop rollout: the joint-space PD law (include/rdyn.h: rdyn_feedback, rdyn_rollout_feedback) and the
model-based laws around it (rdyn_model_feedback, rdyn_rollout_model_feedback)."""


class Feedback(object):
    """u = tau + kp (q_ref - q) + kd (Dq_ref - Dq), clamped to +-tau_limit, as Chain.rollout(feedback=) applies it: `tau` of the rollout
    becomes the feed-forward term.  Everything is in INPUT joint order.
    q_ref, Dq_ref: (T, N, n) for layout="sample", (T, n, N) for "element", one record per step (T at least the rollout's n_steps); or
    shaped like q0, (N, n) / (n, N): a constant set point.  Dq_ref None: zero.
    kp, kd: (n,) shared by all samples, or shaped like q0: per sample.  kd None: no velocity term.
    hold: True, a digital controller: the command is formed once per step from the state at the start of the step and held over the
    integrator's stages; False, the continuous law: formed at every stage at the stage's own state.
    tau_limit: None, or (n,) positive actuator limits; components and wrenches are applied behind the clamp.
    command_trajectory: with trajectory_every >= 1 the rollout also returns the command trajectory, as its last tensor: record r = the
    command of the first evaluation of the step whose end state is state record r."""

    def __init__(self, q_ref, kp, kd=None, Dq_ref=None, hold=True, tau_limit=None, command_trajectory=False):
        self.q_ref, self.Dq_ref, self.kp, self.kd = q_ref, Dq_ref, kp, kd
        self.hold, self.tau_limit, self.command_trajectory = bool(hold), tau_limit, bool(command_trajectory)


class ModelFeedback(Feedback):
    """A model-based law, as Chain.rollout(feedback=) applies it: the controller's own model of the arm inside the loop.
    model: a Chain with the plant's joints and input joints -- Chain.withParameters makes "the same arm with other inertial parameters";
    it may be the plant itself.  RNEA_m below is model.getJointTorque.
    law: "computed_torque": a = DDq_ref + kp (q_ref - q) + kd (Dq_ref - Dq), u = tau + RNEA_m(q, Dq, a), clamped (kp in 1/s^2, kd in
    1/s); "gravity_compensation": u = tau + kp (q_ref - q) + kd (Dq_ref - Dq) + RNEA_m(q, 0, 0), clamped.
    DDq_ref: computed torque only; shaped like q_ref (per step, or a constant record), None: zero.
    Everything else is Feedback's.  Reverse mode is not served yet: Chain.rolloutAdjoint and rosdyn_amd.autograd raise."""

    LAWS = ("computed_torque", "gravity_compensation")

    def __init__(self, model, law, q_ref, kp, kd=None, Dq_ref=None, DDq_ref=None, hold=True, tau_limit=None, command_trajectory=False):
        if law not in self.LAWS:
            raise ValueError("unknown law %r: one of %s" % (law, ", ".join(self.LAWS)))
        if DDq_ref is not None and law != "computed_torque":
            raise ValueError("DDq_ref belongs to the computed-torque law")
        Feedback.__init__(self, q_ref, kp, kd, Dq_ref, hold=hold, tau_limit=tau_limit, command_trajectory=command_trajectory)
        self.model, self.law, self.DDq_ref = model, law, DDq_ref
