"""A closed-loop rollout: Chain.rollout(feedback=Feedback(...)) keeps the controller inside the one-launch horizon (run from the repository
root on a GPU box).  The feed-forward is the computed torque of the MODEL on a smooth reference; the simulated robot is 10 % heavier than
the model.  Open loop the robot leaves the reference within tens of milliseconds; with a joint-space PD law around the same torques it
tracks it over the whole second."""
import math, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rosdyn_amd import Chain, Feedback
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
model = Chain(os.path.join(root, "tests/fixtures/ur10_like.urdf"), "base_link", "tool0", (0, 0, -9.806))
robot = model.withParameters(1.1 * model.getNominalParameters())            # every link 10 % heavier than the model believes
N, T, n, dt, f64 = 256, 1000, model.getActiveJointsNumber(), 1e-3, dict(dtype=torch.float64, device="cuda")
w = 2 * math.pi * (0.2 + 0.4 * torch.rand((N, n), **f64))                   # 0.2 .. 0.6 Hz per joint and sample
arg = torch.arange(T + 1, **f64)[:, None, None] * dt * w + 2 * math.pi * torch.rand((N, n), **f64)
q_ref, Dq_ref, DDq_ref = 0.3 * arg.sin(), 0.3 * w * arg.cos(), -0.3 * w * w * arg.sin()
flat = lambda x: x[:T].reshape(T * N, n)
tau_ff = model.getJointTorque(flat(q_ref), flat(Dq_ref), flat(DDq_ref)).reshape(T, N, n)   # computed torque of the model
m = torch.diagonal(model.getJointInertia(q_ref[0]), dim1=1, dim2=2).mean(dim=0)             # gains from the joints' own inertia:
kp, kd = 100.0 ** 2 * m, 2 * 100.0 * m                                                      # 100 rad/s, critically damped
limit = 1.5 * tau_ff.abs().amax(dim=(0, 1))                                                 # actuators sized 50 % above the model's need
law = Feedback(q_ref[:T].contiguous(), kp, kd, Dq_ref[:T].contiguous(), hold=True, tau_limit=limit)
run = lambda **kw: robot.rollout(q_ref[0].contiguous(), Dq_ref[0].contiguous(), tau_ff, dt, integrator="rk4", trajectory_every=1, **kw)
_, _, st_open, q_open, _ = run()
_, _, st_closed, q_closed, _ = run(feedback=law)
err = lambda q: [float((q[k - 1] - q_ref[k]).abs().max()) for k in (50, 200, T)]
print("status ok:", bool((st_open == 1).all()), bool((st_closed == 1).all()))
print("tracking error (rad) after 50 / 200 / %d steps, open loop  : %.2e %.2e %.2e" % ((T,) + tuple(err(q_open))))
print("tracking error (rad) after 50 / 200 / %d steps, closed loop: %.2e %.2e %.2e" % ((T,) + tuple(err(q_closed))))
