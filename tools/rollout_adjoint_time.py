#!/usr/bin/env python3
"""Timing of the rollout adjoint (rdyn_rollout_adjoint.hip) -> profiles/r14/rollout_adjoint.txt (or the path given; the file is rewritten
after every row, so a run that is cut short keeps what it measured).
One process, one device; medians of REPS interleaved repetitions after warm-up (every repetition runs each leg once, in turn):
  - adjoint   rdyn_rollout_adjoint over the whole horizon: gq0, gdq0 and one torque gradient per step from seeds on the end state;
  - forward   the forward rollout alone (rdyn_rollout with one trajectory record per step), the call whose records the adjoint reads;
  - recipe    semi-implicit Euler only -- what the adjoint replaces there: rdyn_forward_dynamics_derivatives on the trajectory records
              (one call per step on its N records: the 3 n n N doubles of one step, not of the horizon, are resident) and the backward
              recursion stepped on the host with torch (three batched matrix-vector products and the updates per step).  There is no
              such recipe for RK4: the stage states are not exposed.
Shapes: 6 and 7 joints, T = 64, 4 096 / 65 536 / 1e6 samples, both integrators, sample-major."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rosdyn_amd import Chain                                              # noqa: E402

FIXTURES = os.path.join(ROOT, "tests", "fixtures")
GRAV = (0.0, 0.0, -9.806)
REPS = 11
T, DT = 64, 1e-3
lines = []
DST = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r14", "rollout_adjoint.txt")
SIZES = tuple(int(x) for x in sys.argv[2].split(",")) if len(sys.argv) > 2 else (4096, 65536, 1000000)


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
        return Chain(os.path.join(FIXTURES, "ur10_like.urdf"), "base_link", "wrist_3_link", GRAV), 0.4
    return Chain(os.path.join(FIXTURES, "panda_like.urdf"), "link0", "link7", GRAV), 3.0


def measure(name, N, integrator):
    chain, amp = chain_of(name)
    n = chain.getActiveJointsNumber()
    q0, dq0, gq, gv = (torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(4))
    tau = amp * (torch.rand((T, N, n), dtype=torch.float64, device="cuda") * 2 - 1)
    q_end, dq_end, st, q_traj, dq_traj = chain.rollout(q0, dq0, tau, DT, integrator=integrator, trajectory_every=1)
    assert bool((st == 1).all())
    outs = {"gq0": torch.empty_like(q0), "gDq0": torch.empty_like(q0), "gtau": torch.empty_like(tau)}
    mats = {k: torch.empty((N, n, n), dtype=torch.float64, device="cuda") for k in ("dq", "dv", "dtau")}
    mats["ddq"] = torch.empty_like(q0)
    gtau_r = torch.empty_like(tau)

    def recipe():
        lq, lv = gq.clone(), gv.clone()
        for t in range(T - 1, -1, -1):
            q, v = (q0, dq0) if t == 0 else (q_traj[t - 1], dq_traj[t - 1])
            chain.getJointAccelerationDerivatives(q, v, tau[t], out=mats)          # records [s, k, i] = d DDq_i / d x_k
            lv = lv + DT * lq
            mu = (DT * lv).unsqueeze(2)
            lq = lq + torch.bmm(mats["dq"], mu).squeeze(2)
            lv = lv + torch.bmm(mats["dv"], mu).squeeze(2)
            gtau_r[t] = torch.bmm(mats["dtau"], mu).squeeze(2)
        return lq, lv

    legs = {
        "adjoint": lambda: chain.rolloutAdjoint(q0, dq0, tau, DT, q_traj, dq_traj, gq_end=gq, gDq_end=gv, integrator=integrator, out=outs),
        "forward": lambda: chain.rollout(q0, dq0, tau, DT, integrator=integrator, trajectory_every=1),
    }
    if integrator == "semi_implicit_euler":
        legs["recipe"] = recipe
    for _ in range(2):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    if "recipe" in legs:   # the two routes compute the same gradient
        a, r = legs["adjoint"](), recipe()
        scale = float(a[0].abs().max())
        assert float((a[0] - r[0]).abs().max()) <= 1e-9 * scale and float((a[2] - gtau_r).abs().max()) <= 1e-9 * float(a[2].abs().max())
    t = {k: [] for k in legs}
    for _ in range(REPS):
        for k, f in legs.items():
            t[k].append(timed(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    rec = med.get("recipe")
    out("%-11s %3d %8d %-20s %12.1f %12.1f %12s %10.2f %10s" % (name, n, N, integrator, med["adjoint"], med["forward"],
                                                              "%.1f" % rec if rec else "-", med["adjoint"] / med["forward"],
                                                              "%.3f" % (med["adjoint"] / rec) if rec else "-"))
    return med


def main():
    out("T = %d steps, dt = %g; medians of %d interleaved repetitions, microseconds per call" % (T, DT, REPS))
    out("%-11s %3s %8s %-20s %12s %12s %12s %10s %10s" % ("chain", "n", "samples", "integrator", "adjoint", "forward", "recipe", "adj/fwd", "adj/recipe"))
    lost = []
    for N in SIZES:
        for name in ("ur10_like", "panda_like"):
            for integrator in ("semi_implicit_euler", "rk4"):
                m = measure(name, N, integrator)
                if "recipe" in m and m["adjoint"] > m["recipe"]:
                    lost.append("%s N=%d" % (name, N))
    out("")
    out("the adjoint is slower than the Euler recipe it replaces at: %s" % (", ".join(lost) if lost else "no shape measured"))
    out("(recipe: per step rdyn_forward_dynamics_derivatives on the step's N records and three torch.bmm; forward: rdyn_rollout with a record per step)")


if __name__ == "__main__":
    main()
