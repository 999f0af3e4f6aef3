"""Times Chain.rolloutParameterAdjoint (rdyn_rollout_adjoint_parameters) against Chain.rolloutAdjoint (rdyn_rollout_adjoint) on the same
descriptor, and -- semi-implicit Euler only, there is none for RK4 -- against the composition out of the calls the library had before:
per step gtau_t from the adjoint, q̈_t from getJointAcceleration, and Y' w as the `c` output of getRegressorGram with gtau_t in the place
of the measured torque (which pays for a Gram nobody wants).  6 and 7 joints, T = 64, both integrators, 4 096 / 65 536 / 1e6 samples;
medians of 11 into profiles/r15/parameter_gradient.txt.  Run from the repository root on a GPU box:  python tools/parameter_gradient_time.py"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rosdyn_amd import Chain  # noqa: E402

CHAINS = {6: ("tests/fixtures/ur10_like.urdf", "base_link", "tool0"), 7: ("tests/fixtures/panda_like.urdf", "link0", "hand")}
T, DT, REPS = 64, 1e-3, 11


def median_ms(fn):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[REPS // 2]


def main():
    lines = ["parameter gradients of a rollout: T = %d, dt = %g, medians of %d (ms)" % (T, DT, REPS),
             "joints integrator samples | adjoint | adjoint + parameters | ratio | Euler composition | composition / (adjoint + parameters)"]
    for nj, (urdf, base, tool) in CHAINS.items():
        chain = Chain(os.path.join(ROOT, urdf), base, tool, (0.0, 0.0, -9.806))
        n = chain.getActiveJointsNumber()
        for integrator in ("semi_implicit_euler", "rk4"):
            for N in (4096, 65536, 1000000):
                q0, dq0 = (torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(2))
                tau = 10.0 * (torch.rand((T, N, n), dtype=torch.float64, device="cuda") * 2 - 1)
                gq, gv = (torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(2))
                fw = chain.rollout(q0, dq0, tau, DT, integrator=integrator, trajectory_every=1)
                out = {k: torch.empty_like(q0) for k in ("gq0", "gDq0")}
                out["gtau"] = torch.empty_like(tau)
                kw = dict(gq_end=gq, gDq_end=gv, integrator=integrator)
                plain = median_ms(lambda: chain.rolloutAdjoint(q0, dq0, tau, DT, fw[3], fw[4], out=out, **kw))
                pout = dict(out, gpi=torch.empty((10 * chain.getJointsNumber(),), dtype=torch.float64, device="cuda"))
                with_p = median_ms(lambda: chain.rolloutParameterAdjoint(q0, dq0, tau, DT, fw[3], fw[4], out=pout, **kw))
                comp = None
                if integrator == "semi_implicit_euler":
                    def composition():
                        gtau = chain.rolloutAdjoint(q0, dq0, tau, DT, fw[3], fw[4], out=out, **kw)[2]
                        c = None
                        for t in range(T):
                            q, v = (q0, dq0) if t == 0 else (fw[3][t - 1], fw[4][t - 1])
                            ddq, _ = chain.getJointAcceleration(q, v, tau[t])
                            r = chain.getRegressorGram(q, v, ddq, gtau[t])
                            c = r[1] if c is None else c + r[1]
                        return c
                    comp = median_ms(composition)
                lines.append("%d %s %d | %.3f | %.3f | %.2f | %s | %s" % (nj, integrator, N, plain, with_p, with_p / plain,
                                                                          "%.3f" % comp if comp else "-", "%.2f" % (comp / with_p) if comp else "-"))
                print(lines[-1], flush=True)
    os.makedirs(os.path.join(ROOT, "profiles", "r15"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r15", "parameter_gradient.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
