"""Builds libsvs_hip.so (the C-ABI library of hand-written gfx950 kernels) in-tree with hipcc.

    python -m svs_unet_pytorch_amd.build [--force]

hipcc cross-compiles for gfx950 without a GPU; the resulting .so travels to the GPU box with the
repo snapshot (it is git-ignored, not gpurun-ignored).
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libsvs_hip.so")
OBJ = os.path.join(HERE, "build")
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", f"--offload-arch={ARCH}", "-fPIC", "-Wall", "-Wno-unused-function"]


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def _deps():
    hdr = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    hdr.append(os.path.join(os.path.dirname(HERE), "include", "svs_hip.h"))
    return hdr


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


# Per-file flags.  stft.hip / mrstft.hip (complex arithmetic): no SLP vectorisation, i.e. no packed-fp32 instructions.  The
# vectoriser turns complex multiplies into v_pk_mul_f32 / v_pk_fma_f32 with op_sel swizzles, and on gfx950 a packed-fp32
# instruction whose op_sel takes the HIGH half of a source for the low result returns garbage while a bf16 MFMA
# (v_mfma_f32_16x16x32_bf16) of any other wave -- another stream, another process -- is executing on the CU
# (reproduced with two-line kernels: DESIGN.md section 5).  No other source file produces that form; wiener.hip's complex
# arithmetic is fp64, but its fp32 loads and stores sit beside it, so it is built the same way; stretch.hip forms and sums complex
# fp32 sources per lane and is built the same way too (it does not include fft_wave.h), and so is pitch.hip, which does the same
# at four points per source.  f0.hip needs it as well: its arithmetic is fp64 but for ONE fp32 subtraction per term, and a lane forms
# 2, 4 or 8 of those side by side from one broadcast sample and a register window that rotates -- adjacent independent fp32
# subtractions whose operands sit in shuffled registers are exactly what the vectoriser packs with op_sel.  f0_smooth.hip instantiates
# the same device functions (csrc/f0_frame.h) in svs_f0_candidates, whose outputs must be f0.hip's bits: the same flag, the same reason.
EXTRA_FLAGS = {"stft.hip": ["-fno-slp-vectorize"], "mrstft.hip": ["-fno-slp-vectorize"], "wiener.hip": ["-fno-slp-vectorize"],
               "stretch.hip": ["-fno-slp-vectorize"], "pitch.hip": ["-fno-slp-vectorize"], "f0.hip": ["-fno-slp-vectorize"],
               "f0_smooth.hip": ["-fno-slp-vectorize"]}


def _compile(src):
    obj = os.path.join(OBJ, os.path.basename(src)[:-4] + ".o")
    if _stale(obj, [src] + _deps() + [os.path.abspath(__file__)]):
        cmd = ["hipcc", *FLAGS, *EXTRA_FLAGS.get(os.path.basename(src), []), "-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
        if r.stderr.strip():
            sys.stderr.write(r.stderr)
    return obj


def build_lib(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(OBJ, exist_ok=True)
    srcs = sources()
    if force:
        for f in os.listdir(OBJ):
            os.remove(os.path.join(OBJ, f))
    with ThreadPoolExecutor(max_workers=min(6, len(srcs))) as ex:
        objs = list(ex.map(_compile, srcs))
    if force or _stale(LIB, objs):
        cmd = ["hipcc", f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB, *objs]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
        if verbose:
            print(f"built {LIB}")
    elif verbose:
        print(f"{LIB} is up to date")
    return LIB


if __name__ == "__main__":
    build_lib(force="--force" in sys.argv)
