"""A rollout under a tool force: Chain.rollout(ext_wrenches=, ext_link=) keeps the one-launch horizon (run from the repository root on a GPU box).
The wrench [force; torque] acts ON the tool link and is given in the tool's own frame, as getJointTorque(q, Dq, DDq, ext_wrenches_in_link_frame)
takes it; its joint torque depends on q, so it is evaluated at every integrator stage and cannot be folded into tau."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rosdyn_amd import Chain
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
chain = Chain(os.path.join(root, "tests/fixtures/ur10_like.urdf"), "base_link", "tool0", (0, 0, -9.806))
N, T, n, dt = 65_536, 64, chain.getActiveJointsNumber(), 1e-3
q0, Dq0 = (torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(2))
tau = torch.zeros((T, N, n), dtype=torch.float64, device="cuda")
push = torch.zeros((N, 6), dtype=torch.float64, device="cuda")
push[:, 2] = -5.0                                                 # 5 N along -z of the tool frame, held over the horizon
q_free, _, _ = chain.rollout(q0, Dq0, tau, dt, integrator="rk4")
q_push, _, status = chain.rollout(q0, Dq0, tau, dt, integrator="rk4", ext_wrenches=push, ext_link="tool0")
ramp = push[None] * torch.linspace(0, 1, T, dtype=torch.float64, device="cuda")[:, None, None]   # (T, N, 6): one wrench per step
q_ramp, _, _ = chain.rollout(q0, Dq0, tau, dt, integrator="rk4", ext_wrenches=ramp, ext_link="tool0")
print(bool((status == 1).all()), float((q_push - q_free).abs().max()), float((q_ramp - q_free).abs().max()))
