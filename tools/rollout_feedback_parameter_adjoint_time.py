#!/usr/bin/env python3
"""Timing of the adjoint of the closed-loop rollout with parameter gradients (rdyn_rollout_adjoint_fb_params.hip) ->
profiles/r20/rollout_feedback_parameter_adjoint.txt (or the path given; the file is rewritten after every row, so a run that is cut short
keeps what it measured).
One process, one device; medians of REPS interleaved repetitions after warm-up (every repetition runs each leg once, in turn):
  - new      rdyn_rollout_adjoint_feedback_parameters: shared gains, limits, a reference per step; gq0, gdq0, the feed-forward gradient
             and the reference gradients per step, the rows gkp, gkd, glim, and gpi;
  - closed   rdyn_rollout_adjoint_feedback on the same forward call and selection, re-measured in this run;
  - params   rdyn_rollout_adjoint_parameters on the open-loop forward call of the same inputs (gq0, gdq0, gtau per step, gpi), likewise;
  - host     semi-implicit Euler only: the host-stepped composition, getJointAccelerationVjp and getJointAccelerationParameterVjp (the
             sums) per step plus the law's transpose in torch.
Shapes: 6 and 7 joints, T = 64, 4 096 / 65 536 / 1e6 samples, both integrators, both hold modes, sample-major."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rosdyn_amd import Chain, Feedback                                    # noqa: E402

FIXTURES = os.path.join(ROOT, "tests", "fixtures")
GRAV = (0.0, 0.0, -9.806)
REPS = 11
T, DT = 64, 1e-3
lines = []
DST = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r20", "rollout_feedback_parameter_adjoint.txt")
SIZES = tuple(int(x) for x in sys.argv[2].split(",")) if len(sys.argv) > 2 else (4096, 65536, 1000000)
WANT = ("q_ref", "Dq_ref", "kp", "kd", "tau_limit")


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
        return Chain(os.path.join(FIXTURES, "ur10_like.urdf"), "base_link", "wrist_3_link", GRAV), 0.4, 0.1
    return Chain(os.path.join(FIXTURES, "panda_like.urdf"), "link0", "link7", GRAV), 3.0, 0.1


def host_stepped(chain, q0, dq0, tau, traj, law, gq, gv, lim, gpi):
    """semi-implicit Euler: lv* = lv + dt lq; the product and its parameter rows at the command; the law's transpose in torch"""
    q_ref, dq_ref, kp, kd = law
    lq, lv = gq.clone(), gv.clone()
    gkp, gkd, glim = torch.zeros_like(q0), torch.zeros_like(q0), torch.zeros_like(q0)
    gpi.zero_()
    for t in range(T - 1, -1, -1):
        q, v = (q0, dq0) if t == 0 else (traj[0][t - 1], traj[1][t - 1])
        raw = tau[t] + kp * (q_ref[t] - q) + kd * (dq_ref[t] - v)
        u = torch.minimum(torch.maximum(raw, -lim), lim)
        lv = lv + DT * lq
        _, qb, vb, tb = chain.getJointAccelerationVjp(q, v, u, DT * lv)
        gpi += chain.getJointAccelerationParameterVjp(q, v, u, DT * lv, reduce=True)[0]
        g = torch.where((raw > lim) | (raw < -lim), torch.zeros_like(tb), tb)
        lq, lv = lq + qb - kp * g, lv + vb - kd * g
        gkp += (q_ref[t] - q) * g
        gkd += (dq_ref[t] - v) * g
        glim += torch.where(raw > lim, tb, torch.where(raw < -lim, -tb, torch.zeros_like(tb)))
    return lq, lv, gkp, gkd, glim, gpi


def measure(name, N, integrator, hold):
    chain, amp, gain = chain_of(name)
    n = chain.getActiveJointsNumber()
    rnd = lambda *shape: torch.rand(shape, dtype=torch.float64, device="cuda") * 2 - 1
    q0, dq0, gq, gv = (rnd(N, n) for _ in range(4))
    tau = amp * rnd(T, N, n)
    q_ref, dq_ref = q0[None] + 0.5 * rnd(T, N, n), dq0[None] + 0.5 * rnd(T, N, n)
    kp = torch.full((n,), 100.0 * gain * amp, dtype=torch.float64, device="cuda")
    kd = torch.full((n,), 20.0 * gain * amp, dtype=torch.float64, device="cuda")
    lim = torch.full((n,), 10.0 * amp, dtype=torch.float64, device="cuda")
    gpi = torch.empty((10 * chain.getJointsNumber(),), dtype=torch.float64, device="cuda")
    outs = {"gq0": torch.empty_like(q0), "gDq0": torch.empty_like(q0), "gtau": torch.empty_like(tau)}
    law_outs = dict(outs, gq_ref=torch.empty_like(tau), gDq_ref=torch.empty_like(tau), gkp=torch.empty_like(q0), gkd=torch.empty_like(q0),
                    gtau_limit=torch.empty_like(q0))
    r = chain.rollout(q0, dq0, tau, DT, integrator=integrator, trajectory_every=1)
    fb = Feedback(q_ref, kp, kd, dq_ref, hold=hold, tau_limit=lim)
    rf = chain.rollout(q0, dq0, tau, DT, integrator=integrator, trajectory_every=1, feedback=fb)
    assert bool((r[2] == 1).all()) and bool((rf[2] == 1).all())
    kw = dict(gq_end=gq, gDq_end=gv, integrator=integrator)
    nbytes = 8 * N * 10 * chain.getJointsNumber() + 4 * N + (1 << 16)   # the accumulators, the statuses, the sums and their alignment
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    legs = {}
    legs["new"] = lambda: chain.rolloutParameterAdjoint(q0, dq0, tau, DT, rf[3], rf[4], out=dict(law_outs, gpi=gpi), workspace=ws, feedback=fb,
                                                        want_feedback=WANT, **kw)
    legs["closed"] = lambda: chain.rolloutAdjoint(q0, dq0, tau, DT, rf[3], rf[4], out=dict(law_outs), feedback=fb, want_feedback=WANT, **kw)
    legs["params"] = lambda: chain.rolloutParameterAdjoint(q0, dq0, tau, DT, r[3], r[4], out=dict(outs, gpi=gpi), workspace=ws, **kw)
    if integrator == "semi_implicit_euler" and hold:
        legs["host"] = lambda: host_stepped(chain, q0, dq0, tau, (rf[3], rf[4]), (q_ref, dq_ref, kp, kd), gq, gv, lim, gpi)
    for _ in range(2):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(REPS):
        for k, f in legs.items():
            t[k].append(timed(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    ratio = lambda k: "%12.1f %6.2f" % (med[k], med["new"] / med[k])
    host = "%12.1f %6.2f" % (med["host"], med["host"] / med["new"]) if "host" in med else "%12s %6s" % ("-", "-")
    out("%-11s %3d %8d %-20s %4d %12.1f " % (name, n, N, integrator, hold, med["new"]) + " ".join((ratio("closed"), ratio("params"), host)))
    return med


def main():
    out("T = %d steps, dt = %g; medians of %d interleaved repetitions, microseconds per call" % (T, DT, REPS))
    out("x = the new call over rdyn_rollout_adjoint_feedback (closed) and over rdyn_rollout_adjoint_parameters (params); the host-stepped")
    out("composition over the new call (host)")
    out("%-11s %3s %8s %-20s %4s %12s " % ("chain", "n", "samples", "integrator", "hold", "new") + " ".join("%12s %6s" % (k, "x") for k in ("closed", "params", "host")))
    for N in SIZES:
        for name in ("ur10_like", "panda_like"):
            for integrator, hold in (("semi_implicit_euler", True), ("rk4", True), ("rk4", False)):
                measure(name, N, integrator, hold)
    out("")
    out("(semi-implicit Euler is one computation under both hold modes: one row.  new: rdyn_rollout_adjoint_feedback_parameters with shared")
    out(" gains, limits and a reference per step, every law gradient and gpi asked for; host: getJointAccelerationVjp and")
    out(" getJointAccelerationParameterVjp per step and the law's transpose in torch)")


if __name__ == "__main__":
    main()
