#!/usr/bin/env python3
"""Timing of the batched local IK on chains with more than ten input joints (rdyn_long_ik.hip: k_long_ik) -> profiles/r7/long_ik.txt
(or the path given):
  - ms per rdyn_local_ik_damped call at 1e5 and 1e6 poses on generated 14-, 20- and 32-revolute chains and on a 32-joint chain that
    mixes fixed, prismatic and revolute joints (22 input joints); lambda = 1e-3, toll = 1e-6, at most 30 updates, reachable targets
    from seeds displaced by ~0.1 rad;
  - the histogram of the update counts and the statuses;
  - ns per pose update (the call over the sum of the update counts);
  - the kernel's resources from the code object in the built library: VGPRs, scratch, LDS per workgroup, and the waves per SIMD they allow."""
import ctypes
import os
import re
import struct
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.oracle import OracleChain                                     # noqa: E402
from rosdyn_amd import Chain                                              # noqa: E402
from rosdyn_amd._lib import lib                                           # noqa: E402
from rosdyn_amd.samples import uniform_pm1                                # noqa: E402
from rosdyn_amd.urdf_gen import generated_long_chain, generated_revolute_chain  # noqa: E402
from tools.probe import timeit                                            # noqa: E402

lines = []


def out(s):
    print(s, flush=True)
    lines.append(s)


def kernel_resources():
    """VGPRs, SGPRs, scratch and spills of k_long_ik, read from the gfx950 code object inside the built library: its .hip_fatbin
    section holds one clang offload bundle per translation unit; the one that defines k_long_ik is unbundled and its AMDGPU
    metadata note read."""
    llvm = "/opt/rocm/llvm/bin"
    so = os.path.join(ROOT, "rosdyn_amd", "librdyn_hip.so")
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, so, os.path.join(tmp, "so")], check=True)
        data = open(fat, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        start = data.find(magic)
        while start >= 0:
            (n_entries,) = struct.unpack_from("<Q", data, start + len(magic))
            pos = start + len(magic) + 8
            for _ in range(n_entries):
                off, size, id_len = struct.unpack_from("<QQQ", data, pos)
                triple = data[pos + 24:pos + 24 + id_len].decode()
                pos += 24 + id_len
                code = data[start + off:start + off + size]
                if triple.endswith("gfx950") and b"k_long_ik" in code:
                    co = os.path.join(tmp, "co")
                    with open(co, "wb") as f:
                        f.write(code)
                    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                                           text=True).stdout
                    # amdhsa.kernels: one "  - ." entry per kernel of the translation unit
                    meta = [e for e in re.split(r"\n  - ", notes[notes.index("amdhsa.kernels:"):]) if re.search(r"\.name:\s+\S*k_long_ik", e)][0]
                    res = {}
                    for key in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
                        m = re.search(r"\.%s:\s+(\d+)" % key, meta)
                        res[key] = int(m.group(1)) if m else -1
                    return res
            start = data.find(magic, start + len(magic))
    raise RuntimeError("k_long_ik not found in the library's code objects")


def lds_bytes(n):
    """Dynamic LDS of one k_long_ik workgroup, from the library (rdyn_long_ik_lds_bytes, C++ linkage)."""
    f = getattr(lib(), "_Z22rdyn_long_ik_lds_bytesi")
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int]
    return f(n)


def setup(name, N):
    if name == "gen32_mixed":
        xml, tool = generated_long_chain(32, 3232), "l32"
    else:
        nj = int(name[3:])
        xml, tool = generated_revolute_chain(nj, 1000 + nj), "l%d" % nj
    chain, ref = Chain(xml, "l0", tool), OracleChain(xml, "l0", tool)
    n = ref.n
    lo, hi = np.array(ref.spec.q_min), np.array(ref.spec.q_max)
    q_goal = np.clip(uniform_pm1(7, (N, n)), lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo))
    seeds = np.clip(q_goal + 0.1 * uniform_pm1(8, (N, n)), lo, hi)
    tq = torch.from_numpy(np.ascontiguousarray(q_goal.T)).cuda()
    T = chain.getTransformation(tq, layout="element")                  # (4, 3, N)
    ts = torch.from_numpy(np.ascontiguousarray(seeds.T)).cuda()
    return chain, n, T, ts


def main():
    r = kernel_resources()
    vgpr_alloc = -(-r["vgpr_count"] // 8) * 8
    out("k_long_ik (gfx950): %d VGPRs, %d SGPRs, scratch %d B, VGPR spills %d, SGPR spills %d (to VGPR lanes)"
        % (r["vgpr_count"], r["sgpr_count"], r["private_segment_fixed_size"], r["vgpr_spill_count"], r["sgpr_spill_count"]))
    out("lambda = 1e-3, toll = 1e-6, max 30 updates, element-major, targets = FK of goals inside the limits, seeds = goals + 0.1 rad")
    out("%-12s %4s %8s %10s %12s %9s %8s %8s   %s" % ("chain", "n", "poses", "ms/call", "ns/update", "LDS/WG", "waves", "status1",
                                                        "update-count histogram (0, 1, 2, ...)"))
    for name in ("rev14", "rev20", "rev32", "gen32_mixed"):
        for N in (100000, 1000000):
            chain, n, T, ts = setup(name, N)
            sol = torch.empty_like(ts)
            call = lambda: chain.computeLocalIk(T, ts, toll=1e-6, max_iterations=30, damping=1e-3, layout="element", out=sol)
            _, st, it = call()
            t = timeit(call, reps=5, warm=2)
            it = it.cpu().numpy()
            st = st.cpu().numpy()
            lds = lds_bytes(n)
            waves_cu = min((160 * 1024) // lds, 4 * (512 // vgpr_alloc))   # one wave per workgroup
            hist = np.bincount(it, minlength=8)
            out("%-12s %4d %8d %10.3f %12.2f %8.1fK %8.2f %7.1f%%   %s" % (name, n, N, t * 1e3, t / max(1, it.sum()) * 1e9, lds / 1024.0,
                                                                         waves_cu / 4.0, 100.0 * (st == 1).mean(),
                                                                         " ".join(str(x) for x in hist[:12])))
            del sol, T, ts
    out("(waves: per SIMD, from LDS per workgroup (160 KB per CU, one wave per workgroup) and VGPRs (512 per SIMD lane))")


if __name__ == "__main__":
    main()
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r7", "long_ik.txt")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")
