"""Computed-torque control with a wrong model, in one launch: Chain.rollout(feedback=ModelFeedback(model, "computed_torque", ...)) sweeps the
controller's own model of the arm inside the horizon (run from the repository root on a GPU box).  The robot tracks a smooth reference
once with a model whose inertial parameters are 6 % off (every other one too large, the rest too small) and once with the exact model;
with the exact model the error obeys e'' + kd e' + kp e = 0 and decays from the initial offset, with the wrong one the mismatch drives
it."""
import math, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rosdyn_amd import Chain, ModelFeedback
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
robot = Chain(os.path.join(root, "tests/fixtures/ur10_like.urdf"), "base_link", "tool0", (0, 0, -9.806))
pi = robot.getNominalParameters()
wrong = robot.withParameters(pi * (1.0 + 0.06 * np.where(np.arange(pi.size) % 2 == 0, 1.0, -1.0)))   # +-6 % on alternating parameters
N, T, n, dt, f64 = 256, 1000, robot.getActiveJointsNumber(), 1e-3, dict(dtype=torch.float64, device="cuda")
w = 2 * math.pi * (0.2 + 0.4 * torch.rand((N, n), **f64))                   # 0.2 .. 0.6 Hz per joint and sample
arg = torch.arange(T + 1, **f64)[:, None, None] * dt * w + 2 * math.pi * torch.rand((N, n), **f64)
q_ref, Dq_ref, DDq_ref = 0.3 * arg.sin(), 0.3 * w * arg.cos(), -0.3 * w * w * arg.sin()
kp, kd = (torch.full((n,), v, **f64) for v in (50.0 ** 2, 2 * 50.0))        # 50 rad/s, critically damped: 1/s^2 and 1/s
limit = torch.full((n,), 400.0, **f64)
zero = torch.zeros((N, n), **f64)                                           # no feed-forward torque: the law is the whole command
q0 = (q_ref[0] + 0.05).contiguous()                                         # start 0.05 rad off the reference


def run(model, law):
    fb = ModelFeedback(model, law, q_ref[:T].contiguous(), kp, kd, Dq_ref[:T].contiguous(), DDq_ref[:T].contiguous() if law == "computed_torque" else None,
                       hold=True, tau_limit=limit)
    _, _, st, q, _ = robot.rollout(q0, Dq_ref[0].contiguous(), zero, dt, integrator="rk4", n_steps=T, trajectory_every=1, feedback=fb)
    return bool((st == 1).all()), [float((q[k - 1] - q_ref[k]).abs().max()) for k in (50, 200, T)]


for what, model, law in (("computed torque, model 6 % off", wrong, "computed_torque"), ("computed torque, exact model", robot, "computed_torque")):
    ok, err = run(model, law)
    print("%-30s status ok: %s, tracking error (rad) after 50 / 200 / %d steps: %.2e %.2e %.2e" % ((what, ok, T) + tuple(err)))
