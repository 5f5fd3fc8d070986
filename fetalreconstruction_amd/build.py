"""Builds the HIP engine in-tree: fetalreconstruction_amd/lib/libsvr_hip.so (gfx950 only).

hipcc cross-compiles without a GPU; the .so travels to the GPU box with the repo snapshot.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC_DIR = os.path.join(HERE, "csrc")
INC_DIR = os.path.join(os.path.dirname(HERE), "include")
# the translation units of the library; what they #include (csrc/*.inc, csrc/*.h, include/*.h) is found by needs_build's scan
SRC = os.path.join(CSRC_DIR, "svr_hip.hip")            # the engine: every kernel and the C ABI
SRC_SORT = os.path.join(CSRC_DIR, "svr_sort.hip")      # radix sort / prefix sum from hipCUB for its work lists (own translation unit)
SRC_HOST = os.path.join(CSRC_DIR, "svr_host.cpp")      # plain host C++ (the irtkReconstruction mirror)
SRC_PVR_HOST = os.path.join(CSRC_DIR, "pvr_host.cpp")  # the irtkPatchBasedReconstruction loop (host C++)
SRC_IRTK = os.path.join(CSRC_DIR, "irtk_reg.cpp")      # the IRTK registration schedule around the NCC cost (host C++)
SRC_IO = os.path.join(CSRC_DIR, "svr_io.cpp")          # NIfTI-1 reader / writer (zlib)
SRC_RCCL = os.path.join(CSRC_DIR, "svr_rccl.cpp")      # the collectives on RCCL (dlopen: no link-time dependency)
INC = os.path.join(INC_DIR, "svr_hip.h")
INC_HOST = os.path.join(INC_DIR, "svr_host.h")
OUT_DIR = os.path.join(HERE, "lib")
OUT = os.path.join(OUT_DIR, "libsvr_hip.so")
SRC_CLI = os.path.join(CSRC_DIR, "svr_cli.cpp")       # the SVRreconstructionGPU command line (host C++)
SRC_PVR_CLI = os.path.join(CSRC_DIR, "pvr_cli.cpp")   # the PVRreconstructionGPU command line (host C++)
BIN_DIR = os.path.join(HERE, "bin")
CLI = os.path.join(BIN_DIR, "SVRreconstructionGPU")
PVR_CLI = os.path.join(BIN_DIR, "PVRreconstructionGPU")

FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
    # the canonical PSF sequence must be evaluated exactly as written (oracle parity)
    "-ffp-contract=off", "-fno-fast-math",
    # hardware global_atomic_add_f32 for the scatter (coarse-grained hipMalloc memory)
    "-munsafe-fp-atomics",
]


def hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def needs_build():
    """no library, no command lines, or any file under csrc/ or include/ (or this one) newer than the library"""
    if not (os.path.exists(OUT) and os.path.exists(CLI) and os.path.exists(PVR_CLI)):
        return True
    t = os.path.getmtime(OUT)
    files = [__file__] + [os.path.join(d, f) for top in (CSRC_DIR, INC_DIR) for d, _, names in os.walk(top) for f in names]
    return any(os.path.getmtime(f) > t for f in files)


def build(force=False, verbose=False, extra=(), variant=None):
    """variant: tuning builds `lib/libsvr_hip_<variant>.so` with extra -D flags (tools/exp_*.py pick one
    through the SVR_HIP_LIB environment variable); the product is always the un-suffixed library."""
    out = OUT if not variant else os.path.join(OUT_DIR, f"libsvr_hip_{variant}.so")
    if not variant and not force and not needs_build():
        return OUT
    os.makedirs(OUT_DIR, exist_ok=True)
    cmd = [hipcc(), *FLAGS, *extra, "-o", out, SRC, SRC_SORT, SRC_HOST, SRC_PVR_HOST, SRC_IRTK, SRC_IO, SRC_RCCL, "-lz", "-ldl"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    if not variant:
        build_cli(verbose)
    return out


def build_cli(verbose=False):
    """SVRreconstructionGPU and PVRreconstructionGPU: plain host C++ linked against the engine library (found through its rpath)."""
    os.makedirs(BIN_DIR, exist_ok=True)
    cxx = shutil.which("g++") or hipcc()
    for exe, src in ((CLI, SRC_CLI), (PVR_CLI, SRC_PVR_CLI)):
        cmd = [cxx, "-O2", "-std=c++17", "-pthread", "-o", exe, src, "-L" + OUT_DIR, "-lsvr_hip", "-Wl,-rpath,$ORIGIN/../lib"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return CLI


if __name__ == "__main__":
    variant = None
    extra = ["-Rpass-analysis=kernel-resource-usage"] if "--usage" in sys.argv else []
    if "--variant" in sys.argv:
        i = sys.argv.index("--variant")
        variant = sys.argv[i + 1]
        extra += [a for a in sys.argv[i + 2:] if a.startswith("-D")]
    print(build(force="--force" in sys.argv, verbose=True, extra=extra, variant=variant))
