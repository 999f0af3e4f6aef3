#!/usr/bin/env python3
"""Timing of the rollout adjoint with external link wrenches (rdyn_rollout_adjoint_ext.hip) -> profiles/r17/rollout_adjoint_ext.txt (or the
path given; the file is rewritten after every row, so a run that is cut short keeps what it measured).
One process, one device; medians of REPS interleaved repetitions after warm-up (every repetition runs each leg once, in turn):
  - plain      rdyn_rollout_adjoint over the whole horizon, re-measured in this run: gq0, gdq0 and one torque gradient per step from seeds
               on the end state (its forward call has no wrenches);
  - tool       rdyn_rollout_adjoint_ext with a constant wrench on the tool link, the summed wrench gradient asked for;
  - tool, no g the same without the wrench gradient: what the wrench costs the state and torque gradients alone;
  - every      rdyn_rollout_adjoint_ext with a constant wrench on every link, the summed wrench gradient asked for;
  - every/step ... with one wrench record and one gradient record per step.
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
DST = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r17", "rollout_adjoint_ext.txt")
SIZES = tuple(int(x) for x in sys.argv[2].split(",")) if len(sys.argv) > 2 else (4096, 65536, 1000000)
LEGS = ("plain", "tool", "tool, no g", "every", "every/step")


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
    n, L, tool = chain.getActiveJointsNumber(), chain.getLinksNumber(), chain.getLinksName()[-1]
    rnd = lambda *shape: torch.rand(shape, dtype=torch.float64, device="cuda") * 2 - 1
    q0, dq0, gq, gv = (rnd(N, n) for _ in range(4))
    tau = amp * rnd(T, N, n)
    outs = {"gq0": torch.empty_like(q0), "gDq0": torch.empty_like(q0), "gtau": torch.empty_like(tau)}
    legs = {}

    def leg(key, want_ext, sum_ext, **kw):
        r = chain.rollout(q0, dq0, tau, DT, integrator=integrator, trajectory_every=1, **kw)
        assert bool((r[2] == 1).all())
        o = dict(outs)
        if want_ext:
            o["gext"] = torch.empty_like(kw["ext_wrenches"])   # (one record summed over the steps, or one record per step)
        extra = dict(kw, want_ext=want_ext, sum_ext=sum_ext) if kw else {}
        legs[key] = lambda: chain.rolloutAdjoint(q0, dq0, tau, DT, r[3], r[4], gq_end=gq, gDq_end=gv, integrator=integrator, out=o, **extra)

    leg("plain", False, False)
    w_tool = amp * rnd(N, 6)
    leg("tool", True, True, ext_wrenches=w_tool, ext_link=tool)
    leg("tool, no g", False, False, ext_wrenches=w_tool, ext_link=tool)
    leg("every", True, True, ext_wrenches=amp * rnd(N, L, 6))
    if N * L * 6 * T * 16 <= 24 << 30:   # the wrench sequence and its gradient
        leg("every/step", True, False, ext_wrenches=amp * rnd(T, N, L, 6))
    for _ in range(2):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(REPS):
        for k, f in legs.items():
            t[k].append(timed(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    cell = lambda k: "%12.1f %6.2f" % (med[k], med[k] / med["plain"]) if k in med else "%12s %6s" % ("-", "-")
    out("%-11s %3d %8d %-20s %12.1f " % (name, n, N, integrator, med["plain"]) + " ".join(cell(k) for k in LEGS[1:]))
    return med


def main():
    out("T = %d steps, dt = %g; medians of %d interleaved repetitions, microseconds per call; x = the ratio to the plain adjoint" % (T, DT, REPS))
    out("%-11s %3s %8s %-20s %12s " % ("chain", "n", "samples", "integrator", "plain") + " ".join("%12s %6s" % (k, "x") for k in LEGS[1:]))
    for N in SIZES:
        for name in ("ur10_like", "panda_like"):
            for integrator in ("semi_implicit_euler", "rk4"):
                measure(name, N, integrator)
    out("")
    out("(plain: rdyn_rollout_adjoint, no wrenches; tool / every: a constant wrench on the tool link / on every link with the summed wrench")
    out(" gradient; tool, no g: without the wrench gradient; every/step: one wrench record and one gradient record per step)")


if __name__ == "__main__":
    main()
