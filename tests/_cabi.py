"""Test support for the C-ABI tests (no GPU): return codes, descriptors filled with a never-dereferenced address, and the workspace
queries.  Nothing here touches a device: every call either has no samples or fails its checks first."""
import ctypes as C
import os

import _chains
from conftest import GOLDEN


RDYN_OK = 0
RDYN_ERR_INVALID_ARGUMENT = 1
RDYN_ERR_UNSUPPORTED = 5
FAKE = 4096   # never dereferenced: the checks come first
EULER, RK4 = 0, 1


def _rollout_desc(n, N, **kw):
    from rosdyn_amd._lib import RolloutDesc
    d = RolloutDesc()
    d.n_steps, d.integrator, d.dt = 5, RK4, 1e-3
    d.tau, d.tau_step_stride = FAKE, n * N
    d.q_end, d.dq_end, d.q_traj, d.dq_traj = FAKE, FAKE, None, None
    d.traj_step_stride, d.traj_every = 0, 0
    d.status = FAKE
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _query(chain, d, N, chunk_samples=0):
    from rosdyn_amd._lib import lib
    return lib().rdyn_rollout_workspace_bytes(chain._h, C.byref(d), N, chunk_samples)


SWEPT = ["ur10_like", "panda_like", "ur10_public"]
CHUNKED = ["rev11", "rev20", "rev32", "gen20_permuted"]


def _chain(name):
    """the named chain of _chains.py without gravity (it does not enter any check made here)"""
    return _chains._chain(name, gravity=(0.0, 0.0, 0.0))


def _comp(joint=0, ctype=0):
    from rosdyn_amd._lib import Component
    c = Component()
    c.type, c.joint, c.min_velocity, c.max_velocity = ctype, joint, 1e-2, 10.0
    c.parameters[0], c.parameters[1], c.parameters[2] = 1.0, 0.5, 0.0
    return c


def _vjp_query(chain, chunk_samples=0):
    from rosdyn_amd._lib import lib
    return lib().rdyn_forward_dynamics_vjp_workspace_bytes(chain._h, chunk_samples)


def _adjoint_desc(n, N, **kw):
    from rosdyn_amd._lib import RolloutAdjointDesc
    d = RolloutAdjointDesc()
    d.n_steps, d.integrator, d.dt = 5, RK4, 1e-3
    d.tau, d.tau_step_stride = FAKE, n * N
    d.q_traj, d.dq_traj, d.traj_step_stride = FAKE, FAKE, n * N
    d.gq_end, d.gdq_end = FAKE, FAKE
    d.gq_traj, d.gdq_traj, d.gtraj_step_stride = FAKE, FAKE, n * N
    d.gq0, d.gdq0, d.gtau, d.gtau_step_stride = FAKE, FAKE, FAKE, n * N
    d.status = FAKE
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _adj_query(chain, d, N, chunk_samples=0):
    from rosdyn_amd._lib import lib
    return lib().rdyn_rollout_adjoint_workspace_bytes(chain._h, C.byref(d), N, chunk_samples)


def _comps(specs):
    from rosdyn_amd._lib import Component
    arr = (Component * max(len(specs), 1))()
    for a, (ty, joint) in zip(arr, specs):
        a.type, a.joint, a.min_velocity, a.max_velocity = ty, joint, 0.05, 0.8
        a.parameters[:] = [1.0, 0.5, 0.25]
    return arr


def _ext(w=FAKE, link=-1, step_stride=0):
    from rosdyn_amd._lib import ExtWrenches
    x = ExtWrenches()
    x.w, x.link, x.step_stride = w, link, step_stride
    return x


def _batch(N, q=FAKE, dq=FAKE, layout=0):
    from rosdyn_amd._lib import Batch
    b = Batch()
    b.n_samples, b.q, b.dq, b.layout, b.device = N, q, dq, layout, 0
    return b


GOLDEN_FILE = os.path.join(GOLDEN, "dynamics_workspace_bytes.json")
CHUNKS = (0, 1, 64, 1000, 16384)
SAMPLES = (0, 1, 4096)
INTEGRATOR_CODES = (0, 1)   # semi-implicit Euler, RK4


def _query_rollout_desc(integrator):
    from rosdyn_amd._lib import RolloutDesc
    d = RolloutDesc()
    d.n_steps, d.integrator, d.dt, d.tau, d.q_end = 5, integrator, 1e-3, FAKE, FAKE
    return d


def _query_adjoint_desc(integrator):
    from rosdyn_amd._lib import RolloutAdjointDesc
    d = RolloutAdjointDesc()
    d.n_steps, d.integrator, d.dt, d.tau, d.gq0 = 5, integrator, 1e-3, FAKE, FAKE
    return d


def measure(name):
    """Every pinned query of one chain: {query: {key: bytes}}; key = "chunk" or "integrator/n_samples/chunk"."""
    from rosdyn_amd._lib import lib
    chain = _chain(name)   # (kept alive while its handle is in use)
    l, h = lib(), chain._h
    out = {"forward": {}, "derivatives": {}, "vjp": {}, "rollout": {}, "adjoint": {}}
    for chunk in CHUNKS:
        out["forward"][str(chunk)] = l.rdyn_forward_dynamics_workspace_bytes(h, chunk)
        out["derivatives"][str(chunk)] = l.rdyn_forward_dynamics_derivatives_workspace_bytes(h, chunk)
        out["vjp"][str(chunk)] = l.rdyn_forward_dynamics_vjp_workspace_bytes(h, chunk)
        for integrator in INTEGRATOR_CODES:
            rd, ad = _query_rollout_desc(integrator), _query_adjoint_desc(integrator)
            for N in SAMPLES:
                key = "%d/%d/%d" % (integrator, N, chunk)
                out["rollout"][key] = l.rdyn_rollout_workspace_bytes(h, C.byref(rd), N, chunk)
                out["adjoint"][key] = l.rdyn_rollout_adjoint_workspace_bytes(h, C.byref(ad), N, chunk)
    return out
