"""Build tests/device_cpp/limb_dev.hip (test infrastructure; see the head of that file).

    python -m tests.device_cpp.build [--emu] [--force]

build():      hipcc with the library's own flags (distributed_plonk_amd.build.FLAGS) -> tests/device_cpp/_build/liblimb_dev.so, gfx950 code
              for tests/test_gpu_limb_arith.py.  One step from source to shared object: no object file is left behind.
build_emu():  the same file with g++ against the emulated HIP runtime of tests/hostemu -> tests/hostemu/_build/limb/liblimb_emu.so, for
              tests/test_limb_harness_emu.py.
Both rebuild when the file, a csrc header or this script is newer than the output (both outputs are git-ignored).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
SRC = os.path.join(HERE, "limb_dev.hip")
CSRC = os.path.join(ROOT, "distributed_plonk_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "hostemu")
OUT = os.path.join(HERE, "_build", "liblimb_dev.so")
OUT_EMU = os.path.join(EMU, "_build", "limb", "liblimb_emu.so")
COMMAND = "python -m tests.device_cpp.build"


def _newest(extra=()):
    deps = [SRC, os.path.abspath(__file__), *extra] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hpp"))]
    return max(os.path.getmtime(d) for d in deps)


def _fresh(out, newest, force):
    return not force and os.path.exists(out) and os.path.getmtime(out) > newest


def build(force=False, verbose=True):
    from distributed_plonk_amd import build as hip_build
    if _fresh(OUT, max(_newest(), os.path.getmtime(hip_build.__file__)), force):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.check_call([hip_build.HIPCC, *hip_build.FLAGS, "-shared", SRC, "-o", OUT])
    if verbose:
        print("built", OUT)
    return OUT


def build_emu(force=False, verbose=True):
    runtime = [os.path.join(EMU, "hipemu_runtime.cpp"), os.path.join(EMU, "hip", "hip_runtime.h")]
    if _fresh(OUT_EMU, _newest(runtime), force):
        return OUT_EMU
    os.makedirs(os.path.dirname(OUT_EMU), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-pthread", "-shared", "-I", EMU, "-include", "hip/hip_runtime.h", "-Wno-unknown-pragmas",
                           "-Wno-attributes", "-fno-strict-aliasing", "-x", "c++", SRC, runtime[0], "-ldl", "-lrt", "-o", OUT_EMU])
    if verbose:
        print("built", OUT_EMU)
    return OUT_EMU


if __name__ == "__main__":
    (build_emu if "--emu" in sys.argv else build)(force="--force" in sys.argv)
