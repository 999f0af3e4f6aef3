#!/usr/bin/env python3
"""Timing of the batched forward dynamics (rdyn_fwd_dyn.hip) -> profiles/r8/forward_dynamics.txt (or the path given).
One process, one device; medians of 21 interleaved repetitions after warm-up (every repetition runs each leg once, in turn):
  - the new call rdyn_forward_dynamics;
  - the building blocks a caller had before it, on the same inputs: rdyn_joint_inertia + rdyn_joint_torque_nonlinear (M and h written
    to memory, two launches; the solve is not included: a lower bound of the old cost);
  - a plain device copy that moves the call's algorithmic bytes (3 n doubles in, n doubles + 4 B out per sample): the HBM floor;
  - the fp64-issue floor from the kernel's own instruction count: fp64 VALU instructions in the ISA of the instantiation (static count;
    the link loops are unrolled, both sides of a wave-uniform joint-type branch are counted) x 4 cycles per wave64 instruction, over
    1 024 SIMDs at 2.4 GHz.
N = 1e6 at 6 and 7 joints (both layouts), 2e5 at 14 / 20 / 32.  VGPRs, scratch and LDS of every instantiation are read from the code
object inside the built library."""
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
from rosdyn_amd import Chain                                              # noqa: E402
from rosdyn_amd._lib import lib                                           # noqa: E402
from rosdyn_amd.urdf_gen import generated_revolute_chain                     # noqa: E402

FIXTURES = os.path.join(ROOT, "tests", "fixtures")
GRAV = (0.0, 0.0, -9.806)
REPS = 21
lines = []


def out(s):
    print(s, flush=True)
    lines.append(s)


def code_object():
    """The gfx950 code object of rdyn_fwd_dyn.hip inside the built library (its .hip_fatbin section holds one clang offload bundle per
    translation unit): per kernel the resources of the AMDGPU metadata note and the number of fp64 VALU instructions of its ISA."""
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
                if triple.endswith("gfx950") and b"k_fwd_solve" in code:
                    co = os.path.join(tmp, "co")
                    with open(co, "wb") as f:
                        f.write(code)
                    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
                    dis = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
                    res = {}
                    for e in re.split(r"\n  - ", notes[notes.index("amdhsa.kernels:"):]):
                        m = re.search(r"\.name:\s+(\S*k_fwd_\S+)", e)
                        if not m:
                            continue
                        sym = m.group(1)
                        nj = re.search(r"k_fwd_dynILi(\d+)E", sym)
                        key = int(nj.group(1)) if nj else "solve"
                        r = {k: int(re.search(r"\.%s:\s+(\d+)" % k, e).group(1)) for k in
                             ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count")
                             if re.search(r"\.%s:\s+(\d+)" % k, e)}
                        body = dis[dis.index("<%s>:" % sym):]
                        body = body[:body.index("s_endpgm")]
                        r["fp64_valu"] = len(re.findall(r"\bv_(?:fma|mul|add|fmac|rcp|rsq|sqrt|div_\w+|trig_preop|rndne|cvt_i32|ldexp|max|min)_f64", body))
                        r["valu"] = len(re.findall(r"^\s*v_\w+", body, flags=re.M))
                        res[key] = r
                    return res
            start = data.find(magic, start + len(magic))
    raise RuntimeError("rdyn_fwd_dyn.hip not found in the library's code objects")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3   # us


def chain_of(name):
    if name == "ur10_like":
        return Chain(os.path.join(FIXTURES, "ur10_like.urdf"), "base_link", "wrist_3_link", GRAV)
    if name == "panda_like":
        return Chain(os.path.join(FIXTURES, "panda_like.urdf"), "link0", "link7", GRAV)
    nj = int(name[3:])
    return Chain(generated_revolute_chain(nj, 1000 + nj), "l0", "l%d" % nj, GRAV)


def measure(name, N, layout, res):
    chain = chain_of(name)
    n = chain.getActiveJointsNumber()
    shape = (N, n) if layout == "sample" else (n, N)
    q, dq = (torch.rand(shape, dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(2))
    tau = (torch.rand(shape, dtype=torch.float64, device="cuda") * 2 - 1) * 50
    ddq = torch.empty_like(q)
    M = torch.empty((N, n, n) if layout == "sample" else (n, n, N), dtype=torch.float64, device="cuda")
    h = torch.empty_like(q)
    nbytes = lib().rdyn_forward_dynamics_workspace_bytes(chain._h, 0)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda") if nbytes else None
    alg_bytes = N * (4 * n * 8 + 4)
    src = torch.empty((alg_bytes // 16,), dtype=torch.float64, device="cuda")   # a copy reads and writes its size: half the bytes each way
    dst = torch.empty_like(src)
    legs = {
        "new": lambda: chain.getJointAcceleration(q, dq, tau, layout=layout, out=ddq, workspace=ws),
        "old": lambda: (chain.getJointInertia(q, layout=layout, out=M), chain.getJointTorqueNonLinearPart(q, dq, layout=layout, out=h)),
        "M": lambda: chain.getJointInertia(q, layout=layout, out=M),
        "h": lambda: chain.getJointTorqueNonLinearPart(q, dq, layout=layout, out=h),
        "copy": lambda: dst.copy_(src),
    }
    for _ in range(3):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(REPS):
        for k, f in legs.items():
            t[k].append(timed(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    _, st = legs["new"]()
    ok = bool((st == 1).all())
    r = res.get(n if n <= 10 else "solve", {})
    issue = ""
    if n <= 10 and r:
        waves = (N + 63) // 64
        med["issue"] = r["fp64_valu"] * 4.0 * waves / 1024 / 2.4e9 * 1e6
        issue = "%8.1f" % med["issue"]
    out("%-11s %3d %8d %-8s %9.1f %9.1f %8.1f %8.1f %8.1f %9s   %s" % (name, n, N, layout, med["new"], med["old"], med["M"], med["h"], med["copy"],
                                                                  issue or "-", "all solved" if ok else "STATUS != 1"))
    return med


def main():
    res = code_object()
    out("kernel resources (gfx950 code object of rdyn_fwd_dyn.hip):")
    out("%-14s %6s %6s %6s %9s %8s %8s %10s %10s" % ("kernel", "VGPR", "AGPR", "SGPR", "scratch B", "spills", "LDS B", "waves/SIMD", "fp64 VALU"))
    for key in sorted(res, key=lambda k: (isinstance(k, str), k)):
        r = res[key]
        # vgpr_count is the wave's whole allocation in the unified 512-entry file, the AGPR part included
        waves = min(8, 512 // (-(-r["vgpr_count"] // 8) * 8))
        out("%-14s %6d %6d %6d %9d %8d %8d %10d %10d" % ("k_fwd_dyn<%d>" % key if key != "solve" else "k_fwd_solve", r["vgpr_count"], r.get("agpr_count", 0),
                                                       r["sgpr_count"], r["private_segment_fixed_size"], r.get("vgpr_spill_count", 0),
                                                       r["group_segment_fixed_size"], waves, r["fp64_valu"]))
    out("(LDS: static; the sample-major copy-out of k_fwd_dyn adds 64 (n | 1) doubles of dynamic LDS per wave, k_fwd_solve 2 n 64 doubles)")
    out("")
    out("medians of %d interleaved repetitions, microseconds per call" % REPS)
    out("%-11s %3s %8s %-8s %9s %9s %8s %8s %8s %9s" % ("chain", "n", "samples", "layout", "new call", "M + h", "M", "h", "HBM copy", "fp64 issue"))
    verdict = []
    for name, N in (("ur10_like", 1000000), ("panda_like", 1000000)):
        for layout in ("sample", "element"):
            m = measure(name, N, layout, res)
            verdict.append("%s %s: new / (M + h) = %.2f, new / fp64 issue floor = %s, new / HBM copy = %.1f"
                           % (name, layout, m["new"] / m["old"], "%.1f" % (m["new"] / m["issue"]) if m.get("issue") else "-", m["new"] / m["copy"]))
    for name in ("rev14", "rev20", "rev32"):
        m = measure(name, 200000, "element", res)
        verdict.append("%s element: new / (M + h) = %.2f (the in-place factorisation and solves: %.0f us)" % (name, m["new"] / m["old"], m["new"] - m["old"]))
    out("")
    out("expectation 'at <= 10 joints the fused call costs no more than M + h': %s"
        % ("confirmed" if all(float(v.split("= ")[1].split(",")[0]) <= 1.0 for v in verdict[:4]) else
           "REFUTED -- the fused kernel holds more registers than either parent (one wave per SIMD at 6 and 7 joints, see the table above)"
           " and runs well above its fp64 issue floor: latency bound, not HBM bound"))
    for v in verdict:
        out("  " + v)
    out("(M + h: rdyn_joint_inertia + rdyn_joint_torque_nonlinear back to back, what a caller paid before any solve; HBM copy: a device copy")
    out(" of the call's algorithmic bytes, 3 n doubles in and n doubles + 4 B out per sample; fp64 issue: fp64 VALU instructions x 4 cycles x")
    out(" waves / 1 024 SIMDs / 2.4 GHz)")


if __name__ == "__main__":
    main()
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r8", "forward_dynamics.txt")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")
