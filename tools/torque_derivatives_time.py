#!/usr/bin/env python3
"""Timing of the batched joint-torque derivatives (rdyn_torque_deriv.hip) -> profiles/r9/torque_derivatives.txt (or the path given).
One process, one device; medians of 21 interleaved repetitions after warm-up (every repetition runs each leg once, in turn):
  - the new call rdyn_joint_torque_derivatives with all three outputs (dtau_dq, dtau_dv, M) and with the two derivative matrices alone;
  - what a caller had to do before it for the same information: 4 n launches of rdyn_joint_torque (central differences in q and Dq; the
    perturbed inputs are prepared outside the timed region, the subtraction is not included: a lower bound of the old cost) plus one
    rdyn_joint_inertia;
  - the streaming floor of the call's own traffic: (3 n + 2 n^2) 8 bytes per sample (the two derivative matrices) moved by a plain device
    copy, and the same bytes at the rate the element-major getters reach in profiles/r6/sweep_sheet.txt;
  - the fp64-issue floor from the kernel's own instruction count: fp64 VALU instructions in the ISA of the instantiation (static count;
    everything is unrolled, both sides of a wave-uniform joint-type branch are counted) x 4 cycles per wave64 instruction, over
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
    """The gfx950 code object of rdyn_torque_deriv.hip inside the built library (its .hip_fatbin section holds one clang offload bundle per
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
                if triple.endswith("gfx950") and b"k_long_torque_deriv" in code:
                    co = os.path.join(tmp, "co")
                    with open(co, "wb") as f:
                        f.write(code)
                    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
                    dis = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
                    res = {}
                    for e in re.split(r"\n  - ", notes[notes.index("amdhsa.kernels:"):]):
                        m = re.search(r"\.name:\s+(\S*k_(?:long_)?torque_deriv\S+)", e)
                        if not m:
                            continue
                        sym = m.group(1)
                        nj = re.search(r"k_torque_derivILi(\d+)E", sym)
                        key = int(nj.group(1)) if nj else "long"
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
    raise RuntimeError("rdyn_torque_deriv.hip not found in the library's code objects")


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


GETTER_TBS = 5.0   # TB/s: what the element-major getters reach in profiles/r6/sweep_sheet.txt (getTwist / getDTwist / getDDTwist: 5.0-5.1 algorithmic)


def measure(name, N, layout, res):
    chain = chain_of(name)
    n = chain.getActiveJointsNumber()
    shape = (N, n) if layout == "sample" else (n, N)
    mshape = (N, n, n) if layout == "sample" else (n, n, N)
    q, dq, ddq = (torch.rand(shape, dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(3))
    outs = {k: torch.empty(mshape, dtype=torch.float64, device="cuda") for k in ("dq", "dv", "M")}
    two = {k: outs[k] for k in ("dq", "dv")}
    tau = torch.empty_like(q)
    # the 4 n perturbed inputs of the central differences: two buffers (one +h, one -h per joint would be 4 n buffers of the batch; the
    # launches read the same number of bytes either way)
    qp = q + 1e-4
    alg_bytes = N * (3 * n + 2 * n * n) * 8
    src = torch.empty((alg_bytes // 16,), dtype=torch.float64, device="cuda")   # a copy reads and writes its size: half the bytes each way
    dst = torch.empty_like(src)

    def old():
        for _ in range(2 * n):
            chain.getJointTorque(qp, dq, ddq, layout=layout, out=tau)
        for _ in range(2 * n):
            chain.getJointTorque(q, qp, ddq, layout=layout, out=tau)
        chain.getJointInertia(q, layout=layout, out=outs["M"])

    legs = {
        "new3": lambda: chain.getJointTorqueDerivatives(q, dq, ddq, layout=layout, want=("dq", "dv", "M"), out=outs),
        "new2": lambda: chain.getJointTorqueDerivatives(q, dq, ddq, layout=layout, want=("dq", "dv"), out=two),
        "old": old,
        "tau": lambda: chain.getJointTorque(q, dq, ddq, layout=layout, out=tau),
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
    med["stream"] = alg_bytes / (GETTER_TBS * 1e12) * 1e6
    r = res.get(n if n <= 10 else "long", {})
    issue = ""
    if n <= 10 and r:
        waves = (N + 63) // 64
        med["issue"] = r["fp64_valu"] * 4.0 * waves / 1024 / 2.4e9 * 1e6
        issue = "%8.1f" % med["issue"]
    out("%-11s %3d %8d %-8s %9.1f %9.1f %10.1f %8.1f %8.1f %8.1f %9s" % (name, n, N, layout, med["new3"], med["new2"], med["old"], med["tau"], med["copy"],
                                                                       med["stream"], issue or "-"))
    return med


def main():
    res = code_object()
    out("kernel resources (gfx950 code object of rdyn_torque_deriv.hip):")
    out("%-22s %6s %6s %6s %9s %8s %8s %10s %10s" % ("kernel", "VGPR", "AGPR", "SGPR", "scratch B", "spills", "LDS B", "waves/SIMD", "fp64 VALU"))
    for key in sorted(res, key=lambda k: (isinstance(k, str), k)):
        r = res[key]
        # vgpr_count is the wave's whole allocation in the unified 512-entry file, the AGPR part included
        waves = min(8, 512 // (-(-r["vgpr_count"] // 8) * 8))
        out("%-22s %6d %6d %6d %9d %8d %8d %10d %10d" % ("k_torque_deriv<%d>" % key if key != "long" else "k_long_torque_deriv", r["vgpr_count"],
                                                       r.get("agpr_count", 0), r["sgpr_count"], r["private_segment_fixed_size"], r.get("vgpr_spill_count", 0),
                                                       r["group_segment_fixed_size"], waves, r["fp64_valu"]))
    out("(LDS: static; the sample-major copy-out of k_torque_deriv adds 64 (n n | 1) doubles of dynamic LDS per wave, k_long_torque_deriv")
    out(" 27 nj doubles per sample of its workgroup)")
    out("")
    out("medians of %d interleaved repetitions, microseconds per call" % REPS)
    out("%-11s %3s %8s %-8s %9s %9s %10s %8s %8s %8s %9s" % ("chain", "n", "samples", "layout", "dq+dv+M", "dq+dv", "4n tau + M", "one tau", "HBM copy",
                                                         "getters", "fp64 issue"))
    verdict = []
    for name, N in (("ur10_like", 1000000), ("panda_like", 1000000)):
        for layout in ("sample", "element"):
            m = measure(name, N, layout, res)
            verdict.append("%s %s: new / (4 n tau + M) = %.2f, new (dq + dv) / fp64 issue floor = %s, / HBM copy = %.1f, / getter rate = %.1f"
                           % (name, layout, m["new3"] / m["old"], "%.1f" % (m["new2"] / m["issue"]) if m.get("issue") else "-", m["new2"] / m["copy"],
                              m["new2"] / m["stream"]))
    for name in ("rev14", "rev20", "rev32"):
        for layout in ("sample", "element"):
            m = measure(name, 200000, layout, res)
            verdict.append("%s %s: new / (4 n tau + M) = %.2f, new (dq + dv) / HBM copy = %.1f, / getter rate = %.1f"
                           % (name, layout, m["new3"] / m["old"], m["new2"] / m["copy"], m["new2"] / m["stream"]))
    out("")
    out("expectation 'at 6 and 7 joints the new call costs less than the 4 n + 1 launches it replaces': %s"
        % ("confirmed" if all(float(v.split("= ")[1].split(",")[0]) < 1.0 for v in verdict[:4]) else "REFUTED"))
    for v in verdict:
        out("  " + v)
    out("(4 n tau + M: 2 n + 2 n launches of rdyn_joint_torque and one rdyn_joint_inertia back to back, the differences not formed; HBM copy:")
    out(" a device copy of (3 n + 2 n^2) 8 bytes per sample; getters: the same bytes at %.1f TB/s; fp64 issue: fp64 VALU instructions x 4 cycles" % GETTER_TBS)
    out(" x waves / 1 024 SIMDs / 2.4 GHz)")


if __name__ == "__main__":
    main()
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r9", "torque_derivatives.txt")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")
