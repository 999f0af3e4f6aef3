#!/usr/bin/env python3
"""Timing of the batched rollouts (rdyn_rollout.hip) -> profiles/r10/rollout.txt (or the path given).
The fused call rdyn_rollout against the composition a caller had before it: T x (rdyn_forward_dynamics per stage + torch element-wise
updates of the state), on the same inputs, same stream.  T = 64, sample-major, dt = 1e-3; 6 and 7 joints (ur10_like, panda_like), both
integrators, N = 4 096, 65 536 and 1 000 000; rev14 (the chunked route) at N = 65 536.  Medians of interleaved repetitions after warm-up
(every repetition runs each leg once, in turn; 11 repetitions, 5 at N = 1 000 000).
Every case runs in a child process of its own under `timeout`; the first case that fails or runs out of time ends the run."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_STEPS = 64
DT = 1e-3
CASES = [(name, N, integ) for name in ("ur10_like", "panda_like") for integ in ("semi_implicit_euler", "rk4") for N in (4096, 65536, 1000000)] + \
        [("rev14", 65536, "semi_implicit_euler"), ("rev14", 65536, "rk4")]
LIMIT = 240   # seconds per case


def composed_step(chain, q, dq, tau, integrator, tmp, ws):
    """one step of the host loop: a forward-dynamics launch per stage and framework element-wise kernels for the update (in place)"""
    a, qs, vs, aq, av = tmp
    fd = lambda x, v: chain.getJointAcceleration(x, v, tau, out=a, workspace=ws)
    if integrator == "semi_implicit_euler":
        fd(q, dq)
        dq.add_(a, alpha=DT)
        q.add_(dq, alpha=DT)
        return
    fd(q, dq)                                   # k1 = (dq, a1)
    aq.copy_(dq).mul_(1.0 / 6.0)
    av.copy_(a).mul_(1.0 / 6.0)
    qs.copy_(q).add_(dq, alpha=0.5 * DT)
    vs.copy_(dq).add_(a, alpha=0.5 * DT)
    for w, c in ((1.0 / 3.0, 0.5 * DT), (1.0 / 3.0, DT), (1.0 / 6.0, None)):
        fd(qs, vs)                              # k_i = (vs, a_i)
        aq.add_(vs, alpha=w)
        av.add_(a, alpha=w)
        if c is not None:
            qs.copy_(q).add_(vs, alpha=c)
            vs.copy_(dq).add_(a, alpha=c)
    q.add_(aq, alpha=DT)
    dq.add_(av, alpha=DT)


def run_case(name, N, integrator):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from rosdyn_amd import Chain
    from rosdyn_amd._lib import lib
    from rosdyn_amd.urdf_gen import generated_revolute_chain
    fixtures, grav = os.path.join(ROOT, "tests", "fixtures"), (0.0, 0.0, -9.806)
    if name == "ur10_like":
        chain = Chain(os.path.join(fixtures, "ur10_like.urdf"), "base_link", "wrist_3_link", grav)
    elif name == "panda_like":
        chain = Chain(os.path.join(fixtures, "panda_like.urdf"), "link0", "link7", grav)
    else:
        nj = int(name[3:])
        chain = Chain(generated_revolute_chain(nj, 1000 + nj), "l0", "l%d" % nj, grav)
    n = chain.getActiveJointsNumber()
    reps = 5 if N >= 1000000 else 11
    q0, dq0 = (torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(2))
    tau = (torch.rand((T_STEPS, N, n), dtype=torch.float64, device="cuda") * 2 - 1) * 0.4
    q, dq = torch.empty_like(q0), torch.empty_like(q0)
    tmp = [torch.empty_like(q0) for _ in range(5)]
    nbytes = lib().rdyn_forward_dynamics_workspace_bytes(chain._h, 0)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda") if nbytes else None
    out = (torch.empty_like(q0), torch.empty_like(q0))

    def fused():
        return chain.rollout(q0, dq0, tau, DT, integrator=integrator, out=out)

    def composed():
        q.copy_(q0)
        dq.copy_(dq0)
        for t in range(T_STEPS):
            composed_step(chain, q, dq, tau[t], integrator, tmp, ws)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3   # us

    legs = {"fused": fused, "composed": composed}
    for _ in range(2):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            t[k].append(timed(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    _, _, st = fused()
    composed()
    torch.cuda.synchronize()
    ok = bool((st == 1).all())
    diff = float(max((out[0] - q).abs().max(), (out[1] - dq).abs().max()))
    print("%-11s %3d %8d %-20s %12.1f %12.1f %8.2f   %s, max |fused - composed| %.1e" %
          (name, n, N, integrator, med["fused"], med["composed"], med["composed"] / med["fused"], "all solved" if ok else "STATUS != 1", diff), flush=True)


def main(dst):
    lines = ["rollouts: T = %d steps, dt = %g, sample-major; medians of interleaved repetitions, microseconds per rollout" % (T_STEPS, DT),
             "composed = T x (rdyn_forward_dynamics per stage + torch element-wise updates), the composition available before rdyn_rollout",
             "%-11s %3s %8s %-20s %12s %12s %8s" % ("chain", "n", "samples", "integrator", "fused", "composed", "speed-up")]
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
    rows = [l.split() for l in lines[3:] if "all solved" in l or "STATUS" in l]
    if rc == 0 and rows:
        slower = [(r[0], r[2], r[3]) for r in rows if float(r[6]) < 1.0]
        small = [float(r[6]) for r in rows if r[2] == "4096"]
        lines.append("")
        lines.append("expectation 'the fused call is no slower than the composition at any of these sizes': %s" %
                     ("confirmed" if not slower else "REFUTED at " + ", ".join("%s N=%s %s" % s for s in slower)))
        lines.append("expectation 'several times faster at N = 4 096': speed-ups %s" % ", ".join("%.1f" % s for s in small))
        print("\n".join(lines[-2:]), flush=True)
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--case":
        run_case(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    else:
        sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r10", "rollout.txt")))
