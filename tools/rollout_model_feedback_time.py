#!/usr/bin/env python3
"""Timing of the closed-loop rollouts under a model-based law (rdyn_rollout_fb_model.hip) -> profiles/r21/rollout_model_feedback.txt (or
the path given).  Four legs per mode on the same inputs, same stream: the PD closed loop rdyn_rollout_feedback (re-measured here: the ratio
is never taken against a stored number), the fused computed-torque and gravity-compensation calls rdyn_rollout_model_feedback with a
model whose parameters are 6 % off, and the host-stepped composition a caller had before: per evaluation whose command is formed anew
torch forms a = DDq_ref + kp (q_ref - q) + kd (Dq_ref - Dq), model.getJointTorque(q, Dq, a), torch adds tau and clamps, then
getJointAcceleration of the plant, then torch element-wise updates of the state.  T = 64, sample-major, dt = 1e-3, shared gains, limits,
per-step references; 6 and 7 joints (ur10_like, panda_like), both integrators, both hold modes, N = 4 096, 65 536 and 1 000 000.  Medians
of 11 interleaved repetitions after warm-up (every repetition runs each leg once, in turn).
Every case runs in a child process of its own under `timeout`; the first case that fails or runs out of time ends the run."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_STEPS = 64
DT = 1e-3
REPS = 11
CASES = [(name, N, integ) for name in ("ur10_like", "panda_like") for integ in ("semi_implicit_euler", "rk4") for N in (4096, 65536, 1000000)]
LIMIT = 300   # seconds per case


def run_case(name, N, integrator):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from rosdyn_amd import Chain, Feedback, ModelFeedback
    fixtures, grav = os.path.join(ROOT, "tests", "fixtures"), (0.0, 0.0, -9.806)
    if name == "ur10_like":
        chain = Chain(os.path.join(fixtures, "ur10_like.urdf"), "base_link", "wrist_3_link", grav)
    else:
        chain = Chain(os.path.join(fixtures, "panda_like.urdf"), "link0", "link7", grav)
    n = chain.getActiveJointsNumber()
    pi0 = chain.getNominalParameters()
    model = chain.withParameters(pi0 * (1.0 + 0.06 * np.where(np.arange(pi0.size) % 2 == 0, 1.0, -1.0)))
    rand = lambda *shape: torch.rand(shape, dtype=torch.float64, device="cuda") * 2 - 1
    q0, dq0 = rand(N, n), rand(N, n)
    tau = rand(T_STEPS, N, n) * 0.4
    q_ref, dq_ref, ddq_ref = q0[None] + 0.5 * rand(T_STEPS, N, n), dq0[None] + 0.5 * rand(T_STEPS, N, n), rand(T_STEPS, N, n)
    kp, kd, lim = (torch.full((n,), v, dtype=torch.float64, device="cuda") for v in (100.0, 20.0, 60.0))
    q, dq, u, e, acc = (torch.empty_like(q0) for _ in range(5))
    a, qs, vs, aq, av = (torch.empty_like(q0) for _ in range(5))
    out = (torch.empty_like(q0), torch.empty_like(q0))
    pds = {hold: Feedback(q_ref, kp, kd, dq_ref, hold=hold, tau_limit=lim) for hold in (True, False)}
    cts = {hold: ModelFeedback(model, "computed_torque", q_ref, kp, kd, dq_ref, ddq_ref, hold=hold, tau_limit=lim) for hold in (True, False)}
    gcs = {hold: ModelFeedback(model, "gravity_compensation", q_ref, kp, kd, dq_ref, hold=hold, tau_limit=lim) for hold in (True, False)}

    def command(t, x, v):
        torch.sub(q_ref[t], x, out=e)
        torch.addcmul(ddq_ref[t], e, kp, out=acc)
        torch.sub(dq_ref[t], v, out=e)
        acc.addcmul_(e, kd)
        model.getJointTorque(x, v, acc, out=u)
        u.add_(tau[t])
        torch.minimum(u, lim, out=u)
        torch.maximum(u, -lim, out=u)

    def composed(hold):
        q.copy_(q0)
        dq.copy_(dq0)
        for t in range(T_STEPS):
            def fd(x, v, first=False):
                if first or not hold:
                    command(t, x, v)
                chain.getJointAcceleration(x, v, u, out=a)
            if integrator == "semi_implicit_euler":
                fd(q, dq, True)
                dq.add_(a, alpha=DT)
                q.add_(dq, alpha=DT)
                continue
            fd(q, dq, True)
            aq.copy_(dq).mul_(1.0 / 6.0)
            av.copy_(a).mul_(1.0 / 6.0)
            qs.copy_(q).add_(dq, alpha=0.5 * DT)
            vs.copy_(dq).add_(a, alpha=0.5 * DT)
            for w, c in ((1.0 / 3.0, 0.5 * DT), (1.0 / 3.0, DT), (1.0 / 6.0, None)):
                fd(qs, vs)
                aq.add_(vs, alpha=w)
                av.add_(a, alpha=w)
                if c is not None:
                    qs.copy_(q).add_(vs, alpha=c)
                    vs.copy_(dq).add_(a, alpha=c)
            q.add_(aq, alpha=DT)
            dq.add_(av, alpha=DT)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3   # us

    legs = {}
    for hold in (True, False):
        for key, fbs in (("pd", pds), ("ct", cts), ("gc", gcs)):
            legs["%s%d" % (key, hold)] = lambda hold=hold, fbs=fbs: chain.rollout(q0, dq0, tau, DT, integrator=integrator, out=out, feedback=fbs[hold])
        legs["composed%d" % hold] = lambda hold=hold: composed(hold)
    for _ in range(2):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(REPS):
        for k, f in legs.items():
            t[k].append(timed(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    for hold in (True, False):
        _, _, st = legs["ct%d" % hold]()
        composed(hold)
        torch.cuda.synchronize()
        ok = bool((st == 1).all())
        diff = float(max((out[0] - q).abs().max(), (out[1] - dq).abs().max()))
        p, f, g, c = (med["%s%d" % (k, hold)] for k in ("pd", "ct", "gc", "composed"))
        print("%-11s %3d %8d %-20s %4d %10.1f %10.1f %10.1f %10.1f %8.2f %8.2f %8.2f   %s, max |fused - composed| %.1e" %
              (name, n, N, integrator, hold, p, f, g, c, f / p, g / p, c / f, "all solved" if ok else "STATUS != 1", diff), flush=True)


def main(dst):
    lines = ["closed-loop rollouts under a model-based law: T = %d steps, dt = %g, sample-major, shared gains, limits, per-step references, the "
             "model's parameters 6 %% off; medians of %d interleaved repetitions, microseconds per rollout" % (T_STEPS, DT, REPS),
             "pd = rdyn_rollout_feedback in the same run; ct / gc = rdyn_rollout_model_feedback, computed torque / gravity compensation; "
             "composed = per evaluation torch forms a, model.getJointTorque, torch clamps, getJointAcceleration, torch updates (computed torque)",
             "%-11s %3s %8s %-20s %4s %10s %10s %10s %10s %8s %8s %8s" % ("chain", "n", "samples", "integrator", "hold", "pd", "ct", "gc", "composed",
                                                                         "ct/pd", "gc/pd", "comp/ct")]
    print("\n".join(lines), flush=True)
    rc = 0
    for name, N, integ in CASES:
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--case", name, str(N), integ],
                           capture_output=True, text=True)
        if r.returncode != 0:
            lines.append("%s N=%d %s: exit status %d, run ended here\n%s" % (name, N, integ, r.returncode, r.stderr[-2000:]))
            print(lines[-1], flush=True)
            rc = 1
            break
        lines.append(r.stdout.rstrip("\n"))
        print(lines[-1], flush=True)
    rows = [l.split() for ln in lines[3:] for l in ln.split("\n") if "all solved" in l or "STATUS" in l]
    if rc == 0 and rows:
        ratio = [float(r[9]) for r in rows]
        gratio = [float(r[10]) for r in rows]
        comp = [float(r[11]) for r in rows]
        lines.append("")
        lines.append("computed torque / PD closed loop: %.2f .. %.2f; gravity compensation / PD closed loop: %.2f .. %.2f" %
                     (min(ratio), max(ratio), min(gratio), max(gratio)))
        lines.append("composition / fused computed-torque call: %.2f .. %.2f (%s)" %
                     (min(comp), max(comp), "the fused call is faster at every size" if min(comp) > 1.0 else "THE FUSED CALL IS NOT FASTER EVERYWHERE"))
        print("\n".join(lines[-2:]), flush=True)
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--case":
        run_case(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    else:
        sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r21", "rollout_model_feedback.txt")))
