"""Closed-loop output-error identification in a few lines: a real arm is only ever excited under its controller, so the candidate model is
simulated UNDER THE SAME PD LAW AND LIMITS and compared with the recorded motion and the recorded commands; the gradient is taken by
loss.backward() through the closed loop (run from the repository root on a GPU box).  The open-loop variant
(output_error_identification.py) drifts away from a controlled robot's measurements within a fraction of a second.
On an MI355X the loss falls by more than an order of magnitude over the 30 iterations; parameters that 32 ms of motion do not excite
(the fixed first link among them) stay where they started, so the parameter distance falls less than the loss."""
import os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rosdyn_amd import Chain, Feedback, autograd
chain = Chain(os.path.join(ROOT, "tests/fixtures/ur10_public.urdf"), "base_link", "tool0", (0, 0, -9.806))   # 9 chain joints, 6 input joints
N, T, dt, n = 4096, 32, 1e-3, chain.getActiveJointsNumber()
g = torch.Generator(device="cuda").manual_seed(7)
rand = lambda *shape: torch.rand(shape, dtype=torch.float64, device="cuda", generator=g) * 2 - 1
q0, Dq0 = rand(N, n), rand(N, n)
tau_ff = torch.zeros((T, N, n), dtype=torch.float64, device="cuda")                                           # no feed-forward: the controller does the work
q_ref, Dq_ref = q0 + 0.5 * rand(T, N, n), 0.5 * rand(T, N, n)                                                  # the tracking task: a reference per step
kp, kd = torch.full((n,), 20.0, dtype=torch.float64, device="cuda"), torch.full((n,), 2.0, dtype=torch.float64, device="cuda")   # well inside the explicit integrator's stability on the light wrist links
limit = torch.full((n,), 6.0, dtype=torch.float64, device="cuda")                                            # actuator limits: part of the commands saturate
law = Feedback(q_ref, kp, kd, Dq_ref, hold=True, tau_limit=limit, command_trajectory=True)                    # a digital controller, the command record returned last
_, _, _, q_meas, Dq_meas, u_meas = chain.rollout(q0, Dq0, tau_ff, dt, trajectory_every=1, feedback=law)       # the "measurement": the true chain under its controller
print("%.0f %% of the recorded commands sit at a limit" % (100.0 * float((u_meas.abs() == limit).double().mean())))
pi_true = torch.from_numpy(chain.getNominalParameters())
pi_start = pi_true * (1.0 + 0.1 * (torch.rand(pi_true.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3)) * 2 - 1))   # a 10 % wrong model
theta = torch.zeros_like(pi_true, requires_grad=True)                                                          # relative corrections: every parameter on its own scale
opt = torch.optim.Adam([theta], lr=0.002)
for it in range(30):
    opt.zero_grad()
    pi = pi_start * (1.0 + theta)
    _, _, q_traj, Dq_traj, u = autograd.closed_loop_rollout(chain, q0, Dq0, tau_ff, dt, law, trajectory=True, parameters=pi)   # the closed loop on chain.withParameters(pi)
    loss = ((q_traj - q_meas) ** 2).mean() + ((Dq_traj - Dq_meas) ** 2).mean() + ((u - u_meas) ** 2).mean() / float(limit[0]) ** 2
    loss.backward()                                                                                            # ONE rolloutParameterAdjoint(feedback=) call: dL/dpi, then the chain rule to theta
    print("iteration %2d  closed-loop loss %.6e  |pi - pi_true| / |pi_true| %.4f" % (it, loss.item(), float((pi.detach() - pi_true).norm() / pi_true.norm())))
    opt.step()
print("recovered parameters (first link: m, m c, I):", (pi_start * (1.0 + theta.detach()))[:10].numpy().round(5))
print("true parameters      (first link: m, m c, I):", pi_true[:10].numpy().round(5))
