"""Builds liblpm_hip.so (hand-written HIP for gfx950) in-tree with hipcc.

The .so lands next to the sources (learnablepoolingmethods_amd/_lib/) so it travels with the
repo snapshot to the GPU box; nothing is JIT-cached outside the tree.
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.path.join(PKG, "_lib")
LIB = os.path.join(LIBDIR, "liblpm_hip.so")
ARCH = "gfx950"
# -packed-fp32-ops: no v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32.  Round 3, tools/determinism_check.py: the low half of a
# compiler-generated v_pk_fma_f32 chain (vlad_bwd_coldots_k_kernel: two dot products sharing one operand) came out wrong by a few per
# cent in ~3 % of training steps when a second process shared the GPU -- same inputs, the same call repeated at once correct, scalar
# v_fmac_f32 never wrong in 440 steps.  (The host pass does not know the feature and says so: filtered below.)
NO_PACKED_FP32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
# LPM_EXTRA_HIPCC_FLAGS: measurement builds only (-DLPM_MEASURE: docs/switches.md); part of the build digest
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function", *NO_PACKED_FP32,
         *os.environ.get("LPM_EXTRA_HIPCC_FLAGS", "").split()]
# per-file extras.  mha_x3: keep the small 16x16 MFMA accumulators in VGPRs (the AGPR form costs a v_accvgpr_read per
# score in a VALU-bound kernel).
EXTRA_FLAGS = {"mha_x3.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"]}


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: cannot build liblpm_hip.so")
    return exe


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def _digest(paths) -> str:
    h = hashlib.sha256()
    for p in sorted(paths):
        with open(p, "rb") as f:
            h.update(p.encode() + b"\0" + f.read())
    h.update(" ".join(FLAGS).encode())
    h.update(repr(sorted(EXTRA_FLAGS.items())).encode())
    return h.hexdigest()


def build(force: bool = False, verbose: bool = True) -> str:
    """Compile every csrc/*.hip for gfx950 and link liblpm_hip.so.  Returns the library path."""
    os.makedirs(LIBDIR, exist_ok=True)
    srcs = sources()
    deps = (srcs + sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h"))
            + [os.path.join(PKG, "..", "include", "lpm_hip.h")])
    stamp = os.path.join(LIBDIR, "build.sha256")
    dig = _digest(deps)
    if not force and os.path.exists(LIB) and os.path.exists(stamp) and open(stamp).read().strip() == dig:
        return LIB
    hipcc = _hipcc()
    objs = []

    def compile_one(src):
        obj = os.path.join(LIBDIR, os.path.basename(src)[:-4] + ".o")
        cmd = [hipcc, *FLAGS, *EXTRA_FLAGS.get(os.path.basename(src), []), "-c", src, "-o", obj]
        if verbose:
            print("[lpm build]", " ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{r.stdout}\n{r.stderr}")
        err = "\n".join(l for l in r.stderr.splitlines() if "'-packed-fp32-ops' is not a recognized feature" not in l)
        if verbose and err.strip():
            print(err, file=sys.stderr)
        return obj

    with ThreadPoolExecutor(max_workers=min(4, len(srcs))) as ex:
        objs = list(ex.map(compile_one, srcs))
    cmd = [hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", *objs, "-o", LIB]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    with open(stamp, "w") as f:
        f.write(dig)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
