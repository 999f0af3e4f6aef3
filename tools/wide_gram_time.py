#!/usr/bin/env python3
"""Timing of the normal equations wider than 111 columns (rdyn_panel_gram.hip) -> profiles/r7/wide_gram.txt (or the path given):
  - rdyn_regressor_gram_wide on generated all-revolute chains of 12, 14, 20 and 32 input joints (ms per 1e5 samples), beside the
    element-major regressor alone (the image writer's share) and the useful TFLOP/s of the Gram part (only the tiles the zero band leaves);
  - rdyn_gram_wide against rdyn_gram on the same 1e6 x 111 matrix (gate: at most 1.5x);
  - whether the panel pairs' re-reads come from the Infinity Cache: the bytes the pairs request per second on a matrix the size of a chunk
    image (fits the 256 MiB cache) and on one 16x larger (does not), against one pass over the same matrix at HBM rate."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rosdyn_amd import Chain                     # noqa: E402
from rosdyn_amd.gram import gram, gram_wide       # noqa: E402
from rosdyn_amd.urdf_gen import generated_revolute_chain  # noqa: E402
from tools.probe import timeit                   # noqa: E402

PEAK, ISSUE = 78.6, 58.0   # TFLOP/s: datasheet fp64 matrix; measured back-to-back issue ceiling at one wave per SIMD (tools/fp64_issue.hip)
PB = 4                      # 16-column blocks per panel (RDYN_PANEL_BLOCKS)
lines = []


def out(s):
    print(s)
    lines.append(s)


def band_tiles(nj, cols):
    """upper 16 x 16 tiles per row block that the zero band of input joint j leaves, summed over the joints"""
    nb = (cols + 1 + 15) // 16
    return sum(sum(nb - rb for rb in range((10 * j) // 16, nb)) for j in range(nj))


def read_blocks(cols):
    """16-column blocks the panel pairs read per row (every pair its two panels), against nb for one pass"""
    nb = (cols + 1 + 15) // 16
    panels = (nb + PB - 1) // PB
    w = [min(PB, nb - PB * i) for i in range(panels)]
    return sum(w[i] if i == j else w[i] + w[j] for j in range(panels) for i in range(j + 1)), nb


out("rdyn_regressor_gram_wide, generated all-revolute chains, tau_meas, sample-major inputs, default chunk")
out("%6s %8s %12s %14s %12s %12s %10s %10s" % ("joints", "N", "ms / 1e5", "regressor only", "gram part", "useful TF", "/ 78.6", "/ issue"))
for nj, N in ((12, 200000), (14, 200000), (20, 100000), (32, 100000)):
    chain = Chain(generated_revolute_chain(nj, 1000 + nj), "l0", "l%d" % nj, (0, 0, -9.806))
    q, dq, ddq, tau = (torch.rand((N, nj), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(4))
    P = 10 * nj
    o = (torch.empty((P, P), dtype=torch.float64, device="cuda"), torch.empty((P,), dtype=torch.float64, device="cuda"),
         torch.empty((1,), dtype=torch.float64, device="cuda"))
    t = timeit(lambda: chain.getRegressorGramWide(q, dq, ddq, tau, out=o), reps=5, warm=2)
    Y = torch.empty((P, nj, N), dtype=torch.float64, device="cuda")
    qe, dqe, ddqe = (x.T.contiguous() for x in (q, dq, ddq))
    ty = timeit(lambda: chain.getRegressor(qe, dqe, ddqe, layout="element", out=Y), reps=5, warm=2)
    del Y
    tg = max(t - ty, 1e-9)
    flops = 2.0 * 256 * 16 * band_tiles(nj, P) * N / 16   # 16 x 16 tile = 2 * 256 * 16 flop per 16 rows
    tf = flops / tg / 1e12
    out("%6d %8d %12.3f %14.3f %12.3f %12.2f %10.2f %10.2f" % (nj, N, t * 1e3 * 1e5 / N, ty * 1e3 * 1e5 / N, tg * 1e3 * 1e5 / N, tf,
                                                             tf / PEAK, tf / ISSUE))
    torch.cuda.empty_cache()

out("")
out("rdyn_gram_wide vs rdyn_gram, 1e6 x 111 column-major matrix + b")
rows, cols = 1000000, 111
A = torch.rand((cols, rows), dtype=torch.float64, device="cuda")
b = torch.rand((rows,), dtype=torch.float64, device="cuda")
tn = timeit(lambda: gram(A, b), reps=10, warm=3)
tw = timeit(lambda: gram_wide(A, b), reps=10, warm=3)
out("rdyn_gram      %8.3f ms" % (tn * 1e3))
out("rdyn_gram_wide %8.3f ms   ratio %.2f (gate <= 1.5)" % (tw * 1e3, tw / tn))
del A, b
torch.cuda.empty_cache()

out("")
out("re-reads of the panel pairs: requested GB/s = bytes the pairs read / time (one pass would read nb blocks per row)")
out("%6s %9s %10s %10s %12s %14s" % ("cols", "rows", "MB", "ms", "pair reads", "requested GB/s"))
for cols in (321, 415):
    for rows in (40000, 640000):
        A = torch.rand((cols, rows), dtype=torch.float64, device="cuda")
        b = torch.rand((rows,), dtype=torch.float64, device="cuda")
        t = timeit(lambda: gram_wide(A, b), reps=5, warm=2)
        rb, nb = read_blocks(cols)
        mb = 8.0 * rows * (cols + 1) / 1e6
        out("%6d %9d %10.0f %10.3f %11.2fx %14.0f" % (cols, rows, mb, t * 1e3, rb / nb, 8.0 * 16 * rb * rows / t / 1e9))
        del A, b
        torch.cuda.empty_cache()

dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r7", "wide_gram.txt")
os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
with open(dst, "w") as f:
    f.write("\n".join(lines) + "\n")
