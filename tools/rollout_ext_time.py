#!/usr/bin/env python3
"""Timing of the rollouts with external link wrenches (rdyn_rollout_ext.hip) -> profiles/r16/rollout_ext.txt (or the path given).
Legs on the same inputs and the same stream:
  tool      rdyn_rollout_ext with a wrench on the tool link alone (link = joints_number; 6 doubles per sample, in registers)
  all       rdyn_rollout_ext with wrenches on every link (link = -1; links x 6 per sample, read per evaluation where a link is swept)
  without   rdyn_rollout on the same inputs: k_rollout<NJ, INTEGRATOR>, whose code object is what it was before the wrenches were added
            (DESIGN.md section 3): the baseline, re-measured in the same run
  composed  the host-stepped composition the fused call replaces (measured for the tool wrench and for all links): per integrator stage
            getJointTorqueExt(q, 0, 0, W) on the zero-gravity chain, tau - tau_E, rdyn_forward_dynamics, and torch element-wise updates
T = 64, sample-major, dt = 1e-3, wrenches held over the horizon; ur10_like and panda_like (6 and 7 joints), both integrators,
N = 4 096, 65 536 and 1 000 000.  Two warm-up rounds, then 11 interleaved repetitions (every repetition runs each leg once, in turn); the
file gives the median of each leg and the ratios of the medians fused / without and composed / fused.  No ratio is fixed in advance.
Every case runs in a child process of its own under `timeout`; the first case that fails or runs out of time ends the run."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_STEPS = 64
DT = 1e-3
REPS = 11
CASES = [(name, N, integ) for name in ("ur10_like", "panda_like") for integ in ("semi_implicit_euler", "rk4") for N in (4096, 65536, 1000000)]
LIMIT = 240   # seconds per case
AMPLITUDE = 0.4


def composed_step(chain, chain0, W, zero, q, dq, tau, integrator, tmp):
    """one step of the host loop: per stage the wrench torque at the stage's q, the subtraction and a forward-dynamics launch, then
    framework element-wise kernels for the update (in place)"""
    a, qs, vs, aq, av, tau_e, rhs = tmp

    def fd(x, v):
        chain0.getJointTorqueExt(x, zero, zero, W, out=tau_e)
        rhs.copy_(tau).sub_(tau_e)
        chain.getJointAcceleration(x, v, rhs, out=a)

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
    fixtures, grav = os.path.join(ROOT, "tests", "fixtures"), (0.0, 0.0, -9.806)
    spec = (os.path.join(fixtures, "ur10_like.urdf"), "base_link", "wrist_3_link") if name == "ur10_like" else \
        (os.path.join(fixtures, "panda_like.urdf"), "link0", "link7")
    chain, chain0 = Chain(*spec, grav), Chain(*spec, (0.0, 0.0, 0.0))
    n, L = chain.getActiveJointsNumber(), chain.getLinksNumber()
    tool = chain.getLinksName()[-1]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1600 + n)
    q0, dq0 = (torch.rand((N, n), dtype=torch.float64, device="cuda", generator=gen) * 2 - 1 for _ in range(2))
    tau = (torch.rand((T_STEPS, N, n), dtype=torch.float64, device="cuda", generator=gen) * 2 - 1) * AMPLITUDE
    W_all = (torch.rand((N, L, 6), dtype=torch.float64, device="cuda", generator=gen) * 2 - 1) * AMPLITUDE
    W_tool = W_all[:, -1].contiguous()
    W_tool_full = torch.zeros_like(W_all)
    W_tool_full[:, -1] = W_tool
    zero = torch.zeros_like(q0)
    q, dq = torch.empty_like(q0), torch.empty_like(q0)
    tmp = [torch.empty_like(q0) for _ in range(7)]
    outs = {k: (torch.empty_like(q0), torch.empty_like(q0)) for k in ("tool", "all", "without")}

    def composed(W):
        q.copy_(q0)
        dq.copy_(dq0)
        for t in range(T_STEPS):
            composed_step(chain, chain0, W, zero, q, dq, tau[t], integrator, tmp)

    legs = {
        "tool": lambda: chain.rollout(q0, dq0, tau, DT, integrator=integrator, out=outs["tool"], ext_wrenches=W_tool, ext_link=tool),
        "all": lambda: chain.rollout(q0, dq0, tau, DT, integrator=integrator, out=outs["all"], ext_wrenches=W_all),
        "without": lambda: chain.rollout(q0, dq0, tau, DT, integrator=integrator, out=outs["without"]),
        "composed_tool": lambda: composed(W_tool_full),
        "composed_all": lambda: composed(W_all),
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3   # us

    for _ in range(2):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(REPS):
        for k, f in legs.items():
            t[k].append(timed(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    _, _, st = legs["all"]()
    composed(W_all)
    torch.cuda.synchronize()
    ok = bool((st == 1).all())
    diff = float(max((outs["all"][0] - q).abs().max(), (outs["all"][1] - dq).abs().max()))
    print("%-11s %2d %8d %-20s | %10.1f | %10.1f | %10.1f | %10.1f | %10.1f | %6.3f | %6.3f | %7.2f | %7.2f | %s, max |all - composed| %.1e" %
          (name, n, N, integrator, med["tool"], med["all"], med["without"], med["composed_tool"], med["composed_all"],
           med["tool"] / med["without"], med["all"] / med["without"], med["composed_tool"] / med["tool"], med["composed_all"] / med["all"],
           "all solved" if ok else "STATUS != 1", diff), flush=True)


def main(dst):
    lines = ["rollouts with external link wrenches: T = %d steps, dt = %g, sample-major, wrenches held over the horizon; microseconds per" % (T_STEPS, DT),
             "rollout, medians of %d interleaved repetitions after two warm-up rounds" % REPS,
             "tool / all = rdyn_rollout_ext with a wrench on the tool link / on every link; without = rdyn_rollout (k_rollout as it was: the baseline);",
             "composed = T x stages x (getJointTorqueExt on the zero-gravity chain + subtract + rdyn_forward_dynamics) + torch element-wise updates",
             "chain, n, samples, integrator | tool | all | without | composed tool | composed all | tool / without | all / without | "
             "composed / tool | composed / all"]
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
    rows = [[c.strip() for c in l.split("|")] for l in lines[5:] if "all solved" in l or "STATUS" in l]
    if rc == 0 and rows:
        col = lambda i: [float(r[i]) for r in rows]
        lines.append("")
        lines.append("tool / without: %.3f .. %.3f; all / without: %.3f .. %.3f; composed / tool: %.2f .. %.2f; composed / all: %.2f .. %.2f "
                     "(no ratio was fixed in advance)" % (min(col(6)), max(col(6)), min(col(7)), max(col(7)), min(col(8)), max(col(8)),
                                                          min(col(9)), max(col(9))))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--case":
        run_case(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    else:
        sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r16", "rollout_ext.txt")))
