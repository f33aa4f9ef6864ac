"""The monocular initialisation (include/hyslam_amd.h: hs_monoinit_*), what can be checked without a GPU: the ctypes structs and numpy dtypes of
hyslam_amd/_native.py against sizeof / offsetof of the header itself (a C program compiled here), the status values, the work area's size against
its carve, the predicate hs_monoinit_check and the refusals that need no handle, and two stand-alone programs of tests/cpp/monoinit_sanitize/
(nothing is loaded into python): the host side under ASan + UBSan (the predicate, "a refused call enqueues nothing" for both forms on a stub
runtime, the carve of the work area), and the kernels' own math — kernels_monoinit.hip compiled for the host — against the LITERAL reference of
tests/ref_monoinit.py bit for bit, hypothesis by hypothesis."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SAN = os.path.join(ROOT, "tests", "cpp", "monoinit_sanitize")

STRUCTS = {
    "hs_monoinit_params": ("MonoinitParams", "MONOINIT_PARAMS_DTYPE", ("fx", "fy", "cx", "cy", "sigma", "max_iterations", "min_triangulated", "min_frac_triangulated",
                                                                       "min_parallax_deg", "_pad", "seed")),
    "hs_monoinit_result": ("MonoinitResult", "MONOINIT_RESULT_DTYPE", ("status", "n_matches", "model", "best_solution", "best_it_h", "best_it_f", "n_triangulated", "_pad",
                                                                       "score_h", "score_f", "rh", "cos_parallax", "H21", "F21", "n_good", "R21", "t21")),
}
CONSTS = ("HS_MONOINIT_TOO_FEW", "HS_MONOINIT_FAILED", "HS_MONOINIT_OK_H", "HS_MONOINIT_OK_F", "HS_MONOINIT_NONFINITE", "HS_MONOINIT_MODEL_NONE", "HS_MONOINIT_MODEL_H",
          "HS_MONOINIT_MODEL_F", "HS_MONOINIT_DRAW_STRIDE", "HS_MONOINIT_MAX_ITERATIONS")


def header_layout():
    os.makedirs(BUILD, exist_ok=True)
    src, exe = os.path.join(BUILD, "monoinit_layout.c"), os.path.join(BUILD, "monoinit_layout")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "hyslam_amd.h"', "int main(void) {"]
    for s, (_, _, fields) in STRUCTS.items():
        lines.append('printf("S %s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['printf("F %s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f) for f in fields]
    lines += ['printf("K %s %%d\\n", (int)%s);' % (k, k) for k in CONSTS]
    lines += ["return 0; }"]
    with open(src, "w") as f:
        f.write("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    sizes, offs, consts = {}, {}, {}
    for ln in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n"):
        w = ln.split()
        if w and w[0] == "S":
            sizes[w[1]] = int(w[2])
        elif w and w[0] == "F":
            offs[w[1], w[2]] = int(w[3])
        elif w and w[0] == "K":
            consts[w[1]] = int(w[2])
    return sizes, offs, consts


def test_structs_and_dtypes_match_the_header():
    import monoinit_host as MH
    import ref_monoinit as R
    from hyslam_amd import _native as N
    sizes, offs, consts = header_layout()
    assert [sizes[s] for s in STRUCTS] == [48, 200]
    for s, (cname, dname, fields) in STRUCTS.items():
        ct, dt = getattr(N, cname), getattr(N, dname)
        assert C.sizeof(ct) == sizes[s] and tuple(f for f, _ in ct._fields_) == fields, s
        assert dt.itemsize == sizes[s] and dt.names == fields, s
        for f in fields:
            assert getattr(ct, f).offset == offs[s, f] and dt.fields[f][1] == offs[s, f], (s, f)
    assert [consts[k] for k in CONSTS] == [N.HS_MONOINIT_TOO_FEW, N.HS_MONOINIT_FAILED, N.HS_MONOINIT_OK_H, N.HS_MONOINIT_OK_F, N.HS_MONOINIT_NONFINITE,
                                           N.HS_MONOINIT_MODEL_NONE, N.HS_MONOINIT_MODEL_H, N.HS_MONOINIT_MODEL_F, N.HS_MONOINIT_DRAW_STRIDE,
                                           N.HS_MONOINIT_MAX_ITERATIONS] == [0, 1, 2, 3, 4, 0, 1, 2, 8, 65535]
    assert (R.TOO_FEW, R.FAILED, R.OK_H, R.OK_F, R.NONFINITE, R.MODEL_NONE, R.MODEL_H, R.MODEL_F, R.DRAW_STRIDE) == (0, 1, 2, 3, 4, 0, 1, 2, 8)
    assert MH.RESULT_DTYPE == N.MONOINIT_RESULT_DTYPE and len(MH.pack_params(R.DEFAULT)) == sizes["hs_monoinit_params"]
    # the chunk constants the cases name are those of hs_monoinit.h, and the Jacobi's sweep cap is the shared one
    import re

    import monoinit_cases as MC
    text = open(os.path.join(ROOT, "hyslam_amd", "csrc", "hs_monoinit.h")).read()
    const = lambda k: int(re.search(r"#define %s (\d+)" % k, text).group(1))
    assert (const("HS_MONO_KEY_CHUNK"), const("HS_MONO_CHI_CHUNK"), const("HS_MONO_RANK_CHUNK")) == (MC.KEY_CHUNK, MC.CHI_CHUNK, MC.RANK_CHUNK)
    sweeps = int(re.search(r"#define HS_JACOBI_SWEEPS (\d+)", open(os.path.join(ROOT, "hyslam_amd", "csrc", "hs_jacobi.h")).read()).group(1))
    assert sweeps == R.SVD_SWEEPS


def test_work_bytes_equal_the_carve():
    """the carve of hs_monoinit.h: N per problem, 48 floats per problem, three words per key point of frame 1, a score and 12 floats per problem, model
    and hypothesis, each rounded to 256, and 256 spare bytes"""
    from hyslam_amd import _native as N
    lib = N.lib()
    up = lambda v: (v + 255) & ~255
    last = 0
    for Q, n1, H in ((0, 0, 0), (1, 0, 1), (1, 9, 1), (1, 65, 12), (3, 86, 12), (2, 4000, 200), (17, 8000, 200)):
        got = int(lib.hs_monoinit_work_bytes(Q, n1, H))
        assert got == up(Q * 4) + up(Q * 192) + 3 * up(n1 * 4) + up(Q * 2 * H * 4) + up(Q * 2 * H * 48) + 256 and got >= last, (Q, n1, H, got)
        last = got
    assert lib.hs_monoinit_work_bytes(-1, -1, -1) == lib.hs_monoinit_work_bytes(0, 0, 0) == 256


def test_the_predicate_and_refusals_that_need_no_handle():
    from hyslam_amd import _native as N
    lib = N.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.hs_monoinit_estimate(None, 1, *[None] * 7, 0, *[None] * 5) == N.HS_ERR_INVALID
    assert lib.hs_monoinit_estimate_device(None, 1, *[None] * 7, 0, *[None] * 7) == N.HS_ERR_INVALID
    par = np.zeros(1, N.MONOINIT_PARAMS_DTYPE)
    par["fx"], par["fy"], par["cx"], par["cy"], par["sigma"], par["max_iterations"], par["min_triangulated"] = 500, 500, 320, 240, 1, 200, 50
    par["min_frac_triangulated"], par["min_parallax_deg"] = 0.9, 1.0
    off1, off2 = np.array([0, 30], np.int64), np.array([0, 40], np.int64)
    k1, k2, m = np.zeros(30, N.KP_DTYPE), np.zeros(40, N.KP_DTYPE), np.zeros(30, np.int32)
    res, ih, jf, p3d, tri = np.zeros(1, N.MONOINIT_RESULT_DTYPE), np.zeros(30, np.uint8), np.zeros(30, np.uint8), np.zeros(90, np.float32), np.zeros(30, np.uint8)
    check = lambda Q=1, pp=par, o1=off1, o2=off2, draws=None, cap=0, device=0, work=None: lib.hs_monoinit_check(
        Q, p(pp), p(o1), p(k1), p(o2), p(k2), p(m), draws, cap, p(res), p(ih), p(jf), p(p3d), p(tri), device, work)
    assert check() is None
    assert check(Q=0) == b"bad argument" and check(cap=1) == b"bad argument" and check(cap=-1) == b"bad argument"
    assert b"non-decreasing" in check(o1=off1[::-1].copy()) and b"non-decreasing" in check(o2=np.array([-1, 40], np.int64))
    assert b"2^31" in check(o1=np.array([0, 1 << 31], np.int64))
    for field, value, word in (("max_iterations", 0, b"max_iterations"), ("max_iterations", 65536, b"max_iterations"), ("sigma", 0.0, b"sigma"),
                               ("sigma", np.inf, b"sigma"), ("fx", 0.0, b"camera"), ("cy", np.nan, b"camera"), ("min_parallax_deg", 0.0, b"min_parallax_deg"),
                               ("min_parallax_deg", -1.0, b"min_parallax_deg"), ("min_parallax_deg", 180.0, b"min_parallax_deg"),
                               ("min_frac_triangulated", np.nan, b"min_frac_triangulated"), ("min_triangulated", -1, b"min_triangulated")):
        bad = par.copy()
        bad[field] = value
        assert word in check(pp=bad), (field, value)
    assert check(device=1) is not None and check(device=1, work=C.c_void_p(4096 + 8)) is not None
    if k1.ctypes.data % 16 == 0 and k2.ctypes.data % 16 == 0:
        assert check(device=1, work=C.c_void_p(4096)) is None


needs_hipcc = pytest.mark.skipif((shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc")) or not os.path.exists(os.path.join(SAN, "..", "host_sanitize", "Makefile")),
                                 reason="needs hipcc (host-only compile) and tests/cpp/host_sanitize/, whose objects it links")


@needs_hipcc
def test_host_side_under_sanitizers():
    """tests/cpp/monoinit_sanitize: a stand-alone program, ASan + UBSan, CPU only"""
    subprocess.check_call(["make", "-s", "-j4", "-C", SAN], timeout=1500)
    r = subprocess.run([os.path.join(SAN, "_build", "monoinit_sanitize")], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "MONOINIT SANITIZE OK" in r.stdout, out[-4000:]
    assert "refusals: 58 refused calls enqueued nothing" in r.stdout and "layout: 80 carves" in r.stdout, out[-4000:]
    assert not any(x in out for x in ("ERROR: AddressSanitizer", "runtime error", "ERROR: LeakSanitizer")), out[-4000:]


@needs_hipcc
def test_kernel_math_on_the_host_equals_the_reference(tmp_path):
    """tests/cpp/monoinit_sanitize/monoinit_host_math: the __host__ __device__ functions of kernels_monoinit.hip — the source the kernels run —
    compiled for the host, under ASan + UBSan, against LITERAL on EVERY case and sweep scene: every hypothesis' score and model of both kinds float
    for float (NaN equal to NaN), then the result record, both masks, p3d and triangulated"""
    import monoinit_cases as MC
    import monoinit_host as MH
    subprocess.check_call(["make", "-s", "-j4", "-C", SAN], timeout=1500)
    everything = dict(MC.cases())
    everything.update(MC.sweep())
    hyps = 0
    for name in sorted(everything):
        c = everything[name]
        ref = MC.run_reference(c)
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        MH.write_problem(src, c)
        r = subprocess.run([os.path.join(SAN, "_build", "monoinit_host_math"), src, dst], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (name, r.stderr[-2000:])
        out = MH.read_output(dst, len(c["kps1"]))
        assert out["N"] == ref["n_matches"] and out["H"] == c["params"]["max_iterations"], name
        hyps += MH.compare_hypotheses(name, out, ref)
        MH.compare(name, out["res"], out["inliers_h"], out["inliers_f"], out["p3d"], out["triangulated"], ref)
    assert hyps > 5000
