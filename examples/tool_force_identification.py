"""Recover a constant tool force from the end state of a rollout by gradient descent (run from the repository root on a GPU box).
rosdyn_amd.autograd.rollout(ext_wrenches=, ext_link=) is differentiable in the wrench: a record shaped like one step's wrench is held
over the horizon and loss.backward() returns the sum over the steps, from ONE Chain.rolloutAdjoint(ext_wrenches=, sum_ext=True) call."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rosdyn_amd import Chain, autograd
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
chain = Chain(os.path.join(root, "tests/fixtures/ur10_like.urdf"), "base_link", "tool0", (0, 0, -9.806))
N, T, n, dt = 256, 32, chain.getActiveJointsNumber(), 2e-3
q0 = torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1
Dq0 = torch.zeros_like(q0)
tau = torch.zeros((T, N, n), dtype=torch.float64, device="cuda")
truth = torch.tensor([1.0, -2.0, -5.0, 0.0, 0.0, 0.0], dtype=torch.float64, device="cuda")       # a force in the tool frame, N
q_meas, Dq_meas, _ = chain.rollout(q0, Dq0, tau, dt, integrator="rk4", ext_wrenches=truth.expand(N, 6).contiguous(), ext_link="tool0")
force = torch.zeros(3, dtype=torch.float64, device="cuda", requires_grad=True)                    # the unknown: one force for the batch
opt = torch.optim.LBFGS([force], lr=1.0, max_iter=30, line_search_fn="strong_wolfe")


def closure():
    opt.zero_grad()
    wrench = torch.cat([force, force.new_zeros(3)]).expand(N, 6)
    q_end, Dq_end = autograd.rollout(chain, q0, Dq0, tau, dt, integrator="rk4", ext_wrenches=wrench, ext_link="tool0")
    loss = ((q_end - q_meas) ** 2).sum() + ((Dq_end - Dq_meas) ** 2).sum()
    loss.backward()
    return loss


opt.step(closure)
print(force.detach().cpu().numpy(), float(closure().detach()))
