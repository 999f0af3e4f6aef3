#!/usr/bin/env python3
"""Timing of the rollouts with friction and spring components (rdyn_rollout_comp.hip) -> profiles/r11/rollout_components.txt (or the path given).
Three legs on the same inputs and the same stream:
  with      rdyn_rollout_components with a component list (k_rollout_comp<NJ, INTEGRATOR>, one launch for the horizon)
  without   the same call with n_comps = 0: it dispatches to k_rollout<NJ, INTEGRATOR>, whose code object is what it was before the
            components were added (the compiler's resource figures of every instantiation are unchanged): the baseline
  composed  the host-stepped composition the fused call replaces: per integrator stage rdyn_components_regressor into a zeroed tau_add,
            tau - tau_add, rdyn_forward_dynamics, and torch element-wise updates of the state
T = 64, sample-major, dt = 1e-3; ur10_like and panda_like (6 and 7 joints), both integrators, N = 4 096, 65 536 and 1 000 000.
Two warm-up rounds, then interleaved repetitions (every repetition runs each leg once, in turn; 15 repetitions, 7 at N = 1 000 000); the
file gives the median and the spread (min .. max) of each leg and the ratios of the medians with / without and composed / with.  No ratio
is fixed in advance.  Every case runs in a child process of its own under `timeout`; the first case that fails or runs out of time ends
the run."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_STEPS = 64
DT = 1e-3
CASES = [(name, N, integ) for name in ("ur10_like", "panda_like") for integ in ("semi_implicit_euler", "rk4") for N in (4096, 65536, 1000000)]
LIMIT = 240   # seconds per case
TAU_AMPLITUDE = 0.4


def component_set(n):
    """a FRICTION1 and a SPRING on joint 0, a FRICTION2 on the last joint, a SPRING on joint 1, a FRICTION1 on joint 2: five of the n joints'
    worth of arithmetic, parameters of the order of the torques"""
    from rosdyn_amd.components import FRICTION1, FRICTION2, SPRING, ComponentSet
    s = TAU_AMPLITUDE
    return ComponentSet([
        dict(type=FRICTION1, joint=0, min_velocity=0.05, max_velocity=0.8, parameters=[0.3 * s, 0.7 * s]),
        dict(type=FRICTION2, joint=n - 1, min_velocity=0.05, max_velocity=0.8, parameters=[0.3 * s, 0.5 * s, -0.6 * s]),
        dict(type=SPRING, joint=1, parameters=[1.1 * s, -0.4 * s]),
        dict(type=SPRING, joint=0, parameters=[-0.8 * s, 0.3 * s]),
        dict(type=FRICTION1, joint=2, min_velocity=0.05, max_velocity=0.8, parameters=[0.2 * s, 0.4 * s]),
    ], n)


def composed_step(chain, cs, q, dq, tau, integrator, tmp):
    """one step of the host loop: per stage the component torque, the subtraction and a forward-dynamics launch, then framework
    element-wise kernels for the update (in place)"""
    a, qs, vs, aq, av, add, rhs = tmp

    def fd(x, v):
        add.zero_()
        tau_add(cs, x, v, add)
        rhs.copy_(tau).sub_(add)
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


def tau_add(cs, q, dq, add):
    """rdyn_components_regressor with C = NULL: only the torque is accumulated (ComponentSet.getRegressor would write the regressor image too)"""
    import ctypes as C
    import torch
    from rosdyn_amd._lib import LAYOUT_SAMPLE_MAJOR, Batch, check, lib
    b = Batch(q.shape[0], q.data_ptr(), dq.data_ptr(), None, LAYOUT_SAMPLE_MAJOR, q.device.index if q.device.index is not None else -1,
              torch.cuda.current_stream(q.device).cuda_stream)
    check(lib().rdyn_components_regressor(C.cast(cs._arr, C.c_void_p), cs.n_comps, cs.n_active, C.byref(b), None, None, add.data_ptr()))


def run_case(name, N, integrator):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from rosdyn_amd import Chain
    fixtures, grav = os.path.join(ROOT, "tests", "fixtures"), (0.0, 0.0, -9.806)
    if name == "ur10_like":
        chain = Chain(os.path.join(fixtures, "ur10_like.urdf"), "base_link", "wrist_3_link", grav)
    else:
        chain = Chain(os.path.join(fixtures, "panda_like.urdf"), "link0", "link7", grav)
    n = chain.getActiveJointsNumber()
    cs = component_set(n)
    reps = 7 if N >= 1000000 else 15
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1100 + n)
    q0, dq0 = (torch.rand((N, n), dtype=torch.float64, device="cuda", generator=gen) * 2 - 1 for _ in range(2))
    tau = (torch.rand((T_STEPS, N, n), dtype=torch.float64, device="cuda", generator=gen) * 2 - 1) * TAU_AMPLITUDE
    q, dq = torch.empty_like(q0), torch.empty_like(q0)
    tmp = [torch.empty_like(q0) for _ in range(7)]
    out_with = (torch.empty_like(q0), torch.empty_like(q0))
    out_without = (torch.empty_like(q0), torch.empty_like(q0))

    def with_components():
        return chain.rollout(q0, dq0, tau, DT, integrator=integrator, out=out_with, components=cs)

    def without():
        return chain.rollout(q0, dq0, tau, DT, integrator=integrator, out=out_without)

    def composed():
        q.copy_(q0)
        dq.copy_(dq0)
        for t in range(T_STEPS):
            composed_step(chain, cs, q, dq, tau[t], integrator, tmp)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3   # us

    legs = {"with": with_components, "without": without, "composed": composed}
    for _ in range(2):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            t[k].append(timed(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    _, _, st = with_components()
    composed()
    torch.cuda.synchronize()
    ok = bool((st == 1).all())
    diff = float(max((out_with[0] - q).abs().max(), (out_with[1] - dq).abs().max()))
    cell = lambda k: "%10.1f (%.1f .. %.1f)" % (med[k], min(t[k]), max(t[k]))
    print("%-11s %2d %8d %-20s | %s | %s | %s | %6.3f | %7.2f | %s, max |with - composed| %.1e" %
          (name, n, N, integrator, cell("with"), cell("without"), cell("composed"), med["with"] / med["without"], med["composed"] / med["with"],
           "all solved" if ok else "STATUS != 1", diff), flush=True)


def main(dst):
    lines = ["rollouts with components: T = %d steps, dt = %g, sample-major, 5 components on 4 joints; microseconds per rollout," % (T_STEPS, DT),
             "median (min .. max) of interleaved repetitions after two warm-up rounds (15 repetitions, 7 at 1 000 000 samples)",
             "with = rdyn_rollout_components; without = the same call with n_comps = 0 (k_rollout as it was: the baseline);",
             "composed = T x stages x (rdyn_components_regressor into tau_add + subtract + rdyn_forward_dynamics) + torch element-wise updates",
             "chain, n, samples, integrator | with | without | composed | with / without | composed / with"]
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
        lines.append("")
        lines.append("with / without: %.3f .. %.3f; composed / with: %.2f .. %.2f (no ratio was fixed in advance; a with / without visibly above 1 "
                     "points at registers, DESIGN.md section 3, not at the tens of flops of the components)" %
                     (min(float(r[4]) for r in rows), max(float(r[4]) for r in rows), min(float(r[5]) for r in rows), max(float(r[5]) for r in rows)))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--case":
        run_case(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    else:
        sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r11", "rollout_components.txt")))
