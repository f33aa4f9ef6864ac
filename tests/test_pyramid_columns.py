"""The pyramid's column records (HsPyrCol: what a lane of a horizontal pass needs, made by the plan per tile column) against the expressions the kernels
evaluated per workgroup before, restated from the x tables — without a GPU.

tests/cpp/test_pyramid_columns.cpp is a stand-alone program under ASan + UBSan (nothing is loaded into python): the library's host code, compiled
host-only as for tests/test_host_sanitizers.py and linked against its stand-in runtime, so the records are read where the handle relocated and uploaded
them.  Sizes: 1920 x 1080, the four shapes of tests/test_gpu_pyramid_combine.py, and 613 x 99 / 1021 x 64, whose level widths leave every remainder
mod 4 (the program itself requires a fused pair with both widths off a multiple of 4)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "cpp", "host_sanitize")
B = os.path.join(DIR, "_build")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-w"]
SIZES = ((1920, 1080), (209, 97), (64, 48), (417, 33), (641, 97), (613, 99), (1021, 64))

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) or not os.path.exists(os.path.join(DIR, "Makefile")),
                                reason="needs hipcc (host-only compile) and tests/cpp/host_sanitize/ (not shipped to GPU boxes)")


def test_every_column_record_equals_what_the_x_tables_give():
    subprocess.check_call(["make", "-s", "-j4", "-C", DIR], timeout=1500)          # the library's objects (host-only) and fatbin_syms.cpp
    with open(os.path.join(ROOT, "hyslam_amd", "csrc", "Makefile")) as f:
        srcs = [x for x in f.read().split("\n") if x.startswith("SRCS")][0].split(":=")[1].split()
    objs = [os.path.join(B, x[:-4] + ".o") for x in srcs]
    obj, exe = os.path.join(B, "test_pyramid_columns.o"), os.path.join(B, "test_pyramid_columns")
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-fno-gpu-sanitize"] + SAN + ["-c", os.path.join(ROOT, "tests", "cpp", "test_pyramid_columns.cpp"), "-o", obj],
                          timeout=600)
    subprocess.check_call([CLANG] + SAN + [obj, os.path.join(DIR, "hip_stub.cpp"), os.path.join(B, "fatbin_syms.cpp")] + objs + ["-o", exe, "-ldl", "-lpthread"], timeout=600)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("HS_")}
    r = subprocess.run([exe] + [str(v) for s in SIZES for v in s], env=clean, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "PYRAMID COLUMNS OK" in r.stdout, out[-4000:]
    assert not any(x in out for x in ("ERROR: AddressSanitizer", "runtime error", "ERROR: LeakSanitizer")), out[-4000:]
    print(r.stdout)
