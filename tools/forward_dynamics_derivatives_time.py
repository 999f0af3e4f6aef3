#!/usr/bin/env python3
"""Timing of the batched forward-dynamics derivatives (rdyn_fwd_dyn_deriv.hip) -> profiles/r13/forward_dynamics_derivatives.txt (or the
path given; the file is rewritten after every row, so a run that is cut short keeps what it measured).
One process, one device; medians of 21 interleaved repetitions after warm-up (every repetition runs each leg once, in turn):
  - fused     rdyn_forward_dynamics_derivatives with all three matrices (dDDq/dq, dDDq/dDq, M^-1) and ddq;
  - recipe    what it replaces: rdyn_forward_dynamics, rdyn_joint_torque_derivatives (dtau_dq, dtau_dv, M) at that ddq,
              torch.linalg.cholesky(M), torch.cholesky_solve on [dtau_dq | dtau_dv | 1] and the negation of the first two blocks; in the
              element-major layout the matrices are first viewed sample-major (permute), as the batched torch solvers need them;
  - launches  the two library launches of the recipe alone (no factorisation, no solves): what the fused call must beat to gain anything
              besides the torch work;
  - copy      a plain device copy of the call's own traffic, (3 n + n + 3 n^2) 8 bytes per sample.
Shapes: 6 and 7 joints at 4 096 / 65 536 / 1e6 samples in both layouts; 14 / 20 / 32 joints at 2e5 samples."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rosdyn_amd import Chain                                              # noqa: E402
from rosdyn_amd._lib import lib                                           # noqa: E402
from rosdyn_amd.urdf_gen import generated_revolute_chain                     # noqa: E402

FIXTURES = os.path.join(ROOT, "tests", "fixtures")
GRAV = (0.0, 0.0, -9.806)
REPS = 21
lines = []
DST = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r13", "forward_dynamics_derivatives.txt")


def out(s):
    print(s, flush=True)
    lines.append(s)
    os.makedirs(os.path.dirname(DST), exist_ok=True)
    with open(DST, "w") as f:
        f.write("\n".join(lines) + "\n")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3   # us


def chain_of(name):
    if name == "ur10_like":
        return Chain(os.path.join(FIXTURES, "ur10_like.urdf"), "base_link", "wrist_3_link", GRAV)
    if name == "panda_like":
        return Chain(os.path.join(FIXTURES, "panda_like.urdf"), "link0", "link7", GRAV)
    nj = int(name[3:])
    return Chain(generated_revolute_chain(nj, 1000 + nj), "l0", "l%d" % nj, GRAV)


def measure(name, N, layout):
    chain = chain_of(name)
    n = chain.getActiveJointsNumber()
    shape = (N, n) if layout == "sample" else (n, N)
    mshape = (N, n, n) if layout == "sample" else (n, n, N)
    q, dq = (torch.rand(shape, dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(2))
    tau = 50.0 * (torch.rand(shape, dtype=torch.float64, device="cuda") * 2 - 1)
    new = {k: torch.empty(mshape, dtype=torch.float64, device="cuda") for k in ("dq", "dv", "dtau")}
    new["ddq"] = torch.empty_like(q)
    old = {k: torch.empty(mshape, dtype=torch.float64, device="cuda") for k in ("dq", "dv", "M")}
    ddq = torch.empty_like(q)
    eye = torch.eye(n, dtype=torch.float64, device="cuda").expand(N, n, n)
    nb = lib().rdyn_forward_dynamics_derivatives_workspace_bytes(chain._h, 0)
    ws = torch.empty((nb,), dtype=torch.uint8, device="cuda") if nb else None
    nb_old = lib().rdyn_forward_dynamics_workspace_bytes(chain._h, 0)
    ws_old = torch.empty((nb_old,), dtype=torch.uint8, device="cuda") if nb_old else None
    alg_bytes = N * (4 * n + 3 * n * n) * 8
    src = torch.empty((alg_bytes // 16,), dtype=torch.float64, device="cuda")   # a copy reads and writes its size: half the bytes each way
    dst = torch.empty_like(src)

    def launches():
        chain.getJointAcceleration(q, dq, tau, layout=layout, out=ddq, workspace=ws_old)
        chain.getJointTorqueDerivatives(q, dq, ddq, layout=layout, want=("dq", "dv", "M"), out=old)

    def recipe():
        launches()
        # records are [s, k, i] (sample-major) or [k, i, s] (element-major): the matrices D[s, i, k] the solver wants
        if layout == "sample":
            Dq, Dv, M = (old[k].transpose(1, 2) for k in ("dq", "dv", "M"))
        else:
            Dq, Dv, M = (old[k].permute(2, 1, 0) for k in ("dq", "dv", "M"))
        L = torch.linalg.cholesky(M)
        X = torch.cholesky_solve(torch.cat((Dq, Dv, eye), dim=2), L)
        X[:, :, :2 * n].neg_()
        return X

    legs = {
        "fused": lambda: chain.getJointAccelerationDerivatives(q, dq, tau, layout=layout, out=new, workspace=ws),
        "recipe": recipe,
        "launches": launches,
        "copy": lambda: dst.copy_(src),
    }
    for _ in range(3):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(REPS):
        for k, f in legs.items():
            t[k].append(timed(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    out("%-11s %3d %8d %-8s %10.1f %10.1f %10.1f %9.1f %9.2f %9.2f %8.1f" % (name, n, N, layout, med["fused"], med["recipe"], med["launches"], med["copy"],
                                                                          med["fused"] / med["recipe"], med["fused"] / med["launches"],
                                                                          med["fused"] / med["copy"]))
    return med


def main():
    out("medians of %d interleaved repetitions, microseconds per call" % REPS)
    out("%-11s %3s %8s %-8s %10s %10s %10s %9s %9s %9s %8s" % ("chain", "n", "samples", "layout", "fused", "recipe", "launches", "HBM copy", "f/recipe",
                                                             "f/launch", "f/copy"))
    lost = []
    for N in (4096, 65536, 1000000):
        for name in ("ur10_like", "panda_like"):
            for layout in ("sample", "element"):
                m = measure(name, N, layout)
                if m["fused"] > m["recipe"]:
                    lost.append("%s N=%d %s" % (name, N, layout))
    for name in ("rev14", "rev20", "rev32"):
        for layout in ("sample", "element"):
            m = measure(name, 200000, layout)
            if m["fused"] > m["recipe"]:
                lost.append("%s N=200000 %s" % (name, layout))
    out("")
    out("the fused call is slower than the recipe it replaces at: %s" % (", ".join(lost) if lost else "no shape measured"))
    out("(recipe: rdyn_forward_dynamics + rdyn_joint_torque_derivatives with M + torch.linalg.cholesky + torch.cholesky_solve on [dtau_dq | dtau_dv | 1];")
    out(" launches: the two library calls of the recipe alone; HBM copy: a device copy of (4 n + 3 n^2) 8 bytes per sample)")


if __name__ == "__main__":
    main()
