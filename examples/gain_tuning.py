"""Gain tuning by gradient descent through a closed-loop rollout: autograd.rollout(feedback=Feedback(...)) is differentiable in the gains,
so a tracking-plus-effort loss over the simulated horizon can be lowered by a few gradient steps on kp, kd (run from the repository root on
a GPU box).  The robot is 10 % heavier than the model whose computed torque is the feed-forward term; the backward of every step is ONE
launch (Chain.rolloutAdjoint(feedback=)), the transpose of the PD law and of its clamp included."""
import math, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rosdyn_amd import Chain, Feedback, autograd
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
model = Chain(os.path.join(root, "tests/fixtures/ur10_public.urdf"), "base_link", "tool0", (0, 0, -9.806))
robot = model.withParameters(1.1 * model.getNominalParameters())            # every link 10 % heavier than the model believes
N, T, n, dt, f64 = 256, 200, model.getActiveJointsNumber(), 1e-3, dict(dtype=torch.float64, device="cuda")
w = 2 * math.pi * (0.2 + 0.4 * torch.rand((N, n), **f64))                   # 0.2 .. 0.6 Hz per joint and sample
arg = torch.arange(T + 1, **f64)[:, None, None] * dt * w + 2 * math.pi * torch.rand((N, n), **f64)
q_ref, Dq_ref, DDq_ref = 0.3 * arg.sin(), 0.3 * w * arg.cos(), -0.3 * w * w * arg.sin()
flat = lambda x: x[:T].reshape(T * N, n)
tau_ff = model.getJointTorque(flat(q_ref), flat(Dq_ref), flat(DDq_ref)).reshape(T, N, n)   # computed torque of the model
m = torch.diagonal(model.getJointInertia(q_ref[0]), dim1=1, dim2=2).mean(dim=0)             # start from soft gains on the joints' own inertia:
log_kp, log_kd = (20.0 ** 2 * m).log().requires_grad_(True), (2 * 20.0 * m).log().requires_grad_(True)   # 20 rad/s, critically damped
limit = 1.5 * tau_ff.abs().amax(dim=(0, 1))                                                 # actuators sized 50 % above the model's need
effort = 1e-4 / float(tau_ff.abs().mean()) ** 2                                             # weight of the feedback effort against rad^2
opt = torch.optim.Adam([log_kp, log_kd], lr=0.2)                                            # (the gains stay positive: their logarithms are tuned)
for it in range(8):
    opt.zero_grad()
    law = Feedback(q_ref[:T].contiguous(), log_kp.exp(), log_kd.exp(), Dq_ref[:T].contiguous(), hold=True, tau_limit=limit, command_trajectory=True)
    q_end, Dq_end, q_traj, Dq_traj, u = autograd.rollout(robot, q_ref[0].contiguous(), Dq_ref[0].contiguous(), tau_ff, dt, integrator="rk4",
                                                         trajectory=True, feedback=law)
    tracking, spent = ((q_traj - q_ref[1:]) ** 2).mean(), effort * ((u - tau_ff) ** 2).mean()
    loss = tracking + spent
    loss.backward()
    print("step %d: loss %.4e (tracking %.4e rad^2, effort %.4e), kp[0] %.1f kd[0] %.2f" % (it, loss.item(), tracking.item(), spent.item(),
                                                                                         log_kp[0].exp().item(), log_kd[0].exp().item()))
    opt.step()
