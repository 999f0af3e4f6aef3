"""Output-error identification in a few lines: refine perturbed inertial parameters against measured TRAJECTORIES, the gradient taken by
loss.backward() through a rollout (run from the repository root on a GPU box).  The equation-error estimate (getRegressorGram + solve)
needs measured accelerations; this loss needs the measured states only."""
import os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rosdyn_amd import Chain, autograd
chain = Chain(os.path.join(ROOT, "tests/fixtures/ur10_public.urdf"), "base_link", "tool0", (0, 0, -9.806))   # 9 chain joints, 6 input joints
N, T, dt, n = 4096, 32, 2e-3, chain.getActiveJointsNumber()
g = torch.Generator(device="cuda").manual_seed(7)
q0, Dq0 = (torch.rand((N, n), dtype=torch.float64, device="cuda", generator=g) * 2 - 1 for _ in range(2))
tau = 20.0 * (torch.rand((T, N, n), dtype=torch.float64, device="cuda", generator=g) * 2 - 1)
_, _, _, q_meas, Dq_meas = chain.rollout(q0, Dq0, tau, dt, trajectory_every=1)                                # the "measurement": the true chain
pi_true = torch.from_numpy(chain.getNominalParameters())
pi_start = pi_true * (1.0 + 0.1 * (torch.rand(pi_true.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3)) * 2 - 1))   # a 10 % wrong model
theta = torch.zeros_like(pi_true, requires_grad=True)                                                          # relative corrections: every parameter on its own scale
opt = torch.optim.Adam([theta], lr=0.005)
for it in range(20):
    opt.zero_grad()
    pi = pi_start * (1.0 + theta)
    _, _, q_traj, Dq_traj = autograd.rollout(chain, q0, Dq0, tau, dt, trajectory=True, parameters=pi)          # the forward runs on chain.withParameters(pi)
    loss = ((q_traj - q_meas) ** 2).mean() + ((Dq_traj - Dq_meas) ** 2).mean()
    loss.backward()                                                                                            # ONE rolloutParameterAdjoint call: dL/dpi, then the chain rule to theta
    print("iteration %2d  trajectory loss %.6e  |pi - pi_true| / |pi_true| %.4f" % (it, loss.item(), float((pi.detach() - pi_true).norm() / pi_true.norm())))
    opt.step()
