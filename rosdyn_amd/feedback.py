"""The joint-space PD feedback law of a closed-loop rollout (include/rdyn.h: rdyn_feedback, rdyn_rollout_feedback)."""


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
