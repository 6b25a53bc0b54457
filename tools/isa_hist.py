#!/usr/bin/env python3
"""Instruction histogram of one kernel of libsvs_hip.so (static count by class):  python tools/isa_hist.py mr_pass_kernel  [lib]

    python tools/isa_hist.py --resources [lib]

prints instead, for EVERY kernel of the library, what its code object's metadata says it occupies: total VGPRs (AGPRs included), AGPRs,
SGPRs, LDS bytes, private-segment (scratch) bytes, and the waves per SIMD that follow on gfx950: registers are allocated in steps
of 8 out of 512 per lane, a CU has 160 KiB of LDS and four SIMDs, at most 8 waves per SIMD.  One line per kernel, sorted by name,
so that two builds can be compared with diff."""
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_isa import LLVM, device_code_objects  # noqa: E402



def resources(lib):
    rows = []
    field = lambda blk, key: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
    with tempfile.TemporaryDirectory() as wd:
        for co in device_code_objects(lib, wd):
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
            blocks = [".agpr_count:" + b for b in re.split(r"\n\s+- \.agpr_count:", notes)[1:]]      # one metadata block per kernel (keys are sorted)
            mangled = [re.search(r"\.name:\s+'?([^\s']+)", b).group(1) for b in blocks]
            names = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.splitlines()
            for blk, name in zip(blocks, names):
                vgpr, agpr, sgpr = field(blk, "vgpr_count"), field(blk, "agpr_count"), field(blk, "sgpr_count")
                lds, scratch, wg = field(blk, "group_segment_fixed_size"), field(blk, "private_segment_fixed_size"), field(blk, "max_flat_workgroup_size")
                name = re.sub(r"^void |\(.*\)$", "", name)
                waves = min(8, 512 // max(8, (vgpr + 7) // 8 * 8))
                if lds:
                    waves = min(waves, (160 * 1024 // lds) * ((wg + 63) // 64) // 4)
                rows.append(f"{name}  vgpr {vgpr}  agpr {agpr}  sgpr {sgpr}  lds {lds}  scratch {scratch}  waves/simd {waves}")
    print("\n".join(sorted(rows)))


if sys.argv[1] == "--resources":
    resources(sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svs_unet_pytorch_amd", "libsvs_hip.so"))
    sys.exit(0)
pat = sys.argv[1]
lib = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svs_unet_pytorch_amd", "libsvs_hip.so")
with tempfile.TemporaryDirectory() as wd:
    for co in device_code_objects(lib, wd):
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", "--demangle", co], capture_output=True, text=True, check=True).stdout
        sym, hist = None, None
        def flush():
            if sym and pat in sym and hist:
                tot = sum(hist.values())
                cls = collections.Counter()
                for k, v in hist.items():
                    c = "valu" if k.startswith("v_") else "ds" if k.startswith("ds_") else "vmem" if k.startswith(("global_", "buffer_", "flat_", "scratch_")) else "salu" if k.startswith("s_") else "other"
                    if k.startswith("v_mfma"): c = "mfma"
                    if k in ("s_waitcnt", "s_nop", "s_barrier"): c = k
                    cls[c] += v
                print(f"{sym[:110]}\n  total {tot}  " + "  ".join(f"{k} {v}" for k, v in cls.most_common()))
                print("  top: " + "  ".join(f"{k} {v}" for k, v in hist.most_common(18)))
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
            if m:
                flush()
                sym, hist = m.group(1), collections.Counter()
                continue
            m = re.match(r"^\s+([a-z_0-9]+)\s", line)
            if m and hist is not None:
                hist[m.group(1)] += 1
        flush()
