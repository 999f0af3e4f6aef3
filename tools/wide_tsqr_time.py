#!/usr/bin/env python3
"""Timing of the R factor of a matrix wider than 112 columns (rdyn_tsqr_wide: column-panel CholeskyQR) -> profiles/r7/wide_tsqr.txt
(or the path given):
  - rdyn_tsqr_wide against rdyn_gram_wide on the same seeded random rows x n1 matrix, n1 = 113 / 200 / 321 / 416, with the stage the
    device accepted;
  - the fixed cost of a call (the dense steps of the accepted round + launches): the intercept of two row counts;
  - the useful rate of the whole call, counted as rows x n1^2 (Q = [A b] W) + rows x n1^2 (its Gram) per round that ran;
  - |R'R - M'M| / |M'M| of every timed factor (M'M through torch on the device)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rosdyn_amd._lib import lib                                      # noqa: E402
from rosdyn_amd.gram import gram_wide, tsqr_wide, tsqr_wide_last_report  # noqa: E402
from tools.probe import timeit                                       # noqa: E402

lines = []


def out(s):
    print(s, flush=True)
    lines.append(s)


def main():
    g = torch.Generator(device="cuda").manual_seed(7)
    out("rdyn_tsqr_wide vs rdyn_gram_wide, seeded normal(0, 1) matrices [A | b] (column-major, lda = rows); ms per call (10 reps after 3)")
    out("%5s %9s %10s %10s %6s %6s %14s %12s %10s" % ("n1", "rows", "tsqr_wide", "gram_wide", "ratio", "stage", "fixed (ms)", "TFLOP/s",
                                                      "R'R err"))
    for n1 in (113, 200, 321, 416):
        P = n1 - 1
        ws = torch.empty((lib().rdyn_tsqr_wide_workspace_bytes(n1),), dtype=torch.uint8, device="cuda")
        t_of = {}
        for rows in (200000, 1000000):
            A = torch.randn((P, rows), dtype=torch.float64, device="cuda", generator=g)
            b = torch.randn((rows,), dtype=torch.float64, device="cuda", generator=g)
            R = torch.empty((n1, n1), dtype=torch.float64, device="cuda")
            t_q = timeit(lambda: tsqr_wide(A, b, out=R, workspace=ws))
            rep = tsqr_wide_last_report(n1, ws)
            t_g = timeit(lambda: gram_wide(A, b))
            At = torch.cat([A, b.view(1, -1)])
            F = At @ At.t()
            err = (torch.linalg.norm(R.t() @ R - F) / torch.linalg.norm(F)).item()
            assert err <= 1e-12, (n1, rows, err)
            del At, F
            t_of[rows] = t_q
            rounds = sum(1 for x in rep["rho"] if x > 0)
            flops = 2.0 * rounds * 2.0 * rows * n1 * n1
            fixed = ""
            if rows == 1000000:
                fixed = "%.3f" % ((t_of[200000] * 1000000 - t_q * 200000) / 800000 * 1e3)
            out("%5d %9d %10.3f %10.3f %6.2f %6d %14s %12.2f %10.1e" % (n1, rows, t_q * 1e3, t_g * 1e3, t_q / t_g, rep["stage"], fixed,
                                                                       flops / t_q * 1e-12, err))
            del A, b
        del ws
    out("(TFLOP/s: 2 x (rows n1^2 of the product + rows n1^2 of its Gram) per round that ran, over the whole call)")


if __name__ == "__main__":
    main()
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r7", "wide_tsqr.txt")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")
