"""The batched Horn Sim3 RANSAC (include/hyslam_amd.h: hs_sim3_*), what can be checked without a GPU: the ctypes structs and numpy dtypes of
hyslam_amd/_native.py against sizeof / offsetof of the header itself (a C program compiled here), the status values, hs_sim3_plan against the
reference's plan over a grid, the work area's size against its carve, the refusals that need no handle, and two stand-alone programs of
tests/cpp/sim3_sanitize/ (nothing is loaded into python): the host side under ASan + UBSan (hs_sim3_plan, "a refused call enqueues nothing" for both
forms on a stub runtime, the carve of the work area), and the kernels' own math — kernels_sim3.hip compiled for the host — against the D19 reference of
tests/ref_sim3.py bit for bit."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SAN = os.path.join(ROOT, "tests", "cpp", "sim3_sanitize")

STRUCTS = {
    "hs_sim3_corr": ("Sim3Corr", "SIM3_CORR_DTYPE", ("X1c", "sigma2_1", "X2c", "sigma2_2", "idx1", "_pad")),
    "hs_sim3_params": ("Sim3Params", "SIM3_PARAMS_DTYPE", ("probability", "min_inliers", "max_iterations", "fix_scale", "_pad", "fx1", "fy1", "cx1", "cy1", "fx2", "fy2",
                                                         "cx2", "cy2", "seed")),
    "hs_sim3_plan_t": ("Sim3Plan", None, ("max_iterations", "epsilon")),
    "hs_sim3_state": ("Sim3State", "SIM3_STATE_DTYPE", ("iterations", "best_inliers", "R", "t", "s", "T12", "_pad")),
    "hs_sim3_result": ("Sim3Result", "SIM3_RESULT_DTYPE", ("T12", "R", "t", "s", "status", "n_inliers", "at_iteration", "iterations", "hypotheses_run")),
}
CONSTS = ("HS_SIM3_TOO_FEW", "HS_SIM3_FOUND", "HS_SIM3_CONTINUE", "HS_SIM3_EXHAUSTED", "HS_SIM3_NONFINITE", "HS_SIM3_DRAW_STRIDE", "HS_SIM3_EIG_SWEEPS")


def header_layout():
    """{struct: sizeof}, {(struct, field): offsetof} and {constant: value}, as a C compiler reads include/hyslam_amd.h"""
    os.makedirs(BUILD, exist_ok=True)
    src, exe = os.path.join(BUILD, "sim3_layout.c"), os.path.join(BUILD, "sim3_layout")
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
    from hyslam_amd import _native as N
    sizes, offs, consts = header_layout()
    assert [sizes[s] for s in STRUCTS] == [48, 64, 8, 128, 136]
    for s, (cname, dname, fields) in STRUCTS.items():
        ct = getattr(N, cname)
        assert C.sizeof(ct) == sizes[s] and tuple(f for f, _ in ct._fields_) == fields, s
        for f in fields:
            assert getattr(ct, f).offset == offs[s, f], (s, f)
        if dname:
            dt = getattr(N, dname)
            assert dt.itemsize == sizes[s] and dt.names == fields, s
            for f in fields:
                assert dt.fields[f][1] == offs[s, f], (s, f)
    assert [consts[k] for k in CONSTS[:6]] == [N.HS_SIM3_TOO_FEW, N.HS_SIM3_FOUND, N.HS_SIM3_CONTINUE, N.HS_SIM3_EXHAUSTED, N.HS_SIM3_NONFINITE, N.HS_SIM3_DRAW_STRIDE] == [0, 1, 2, 3, 4, 4]
    import ref_sim3 as R
    assert R.CORR_DTYPE == N.SIM3_CORR_DTYPE and (R.TOO_FEW, R.FOUND, R.CONTINUE, R.EXHAUSTED, R.NONFINITE, R.DRAW_STRIDE) == (0, 1, 2, 3, 4, 4)
    assert R.EIG_SWEEPS == consts["HS_SIM3_EIG_SWEEPS"]


def test_plan_equals_the_reference_over_a_grid():
    import ref_sim3 as R
    from hyslam_amd import _native as N
    lib = N.lib()
    n = 0
    for prob in (0.0, 0.5, 0.9, 0.99, 0.999999, 1.0, 1.5, -1.0):
        for N_ in (0, 1, 2, 3, 5, 19, 20, 21, 40, 100, 257, 5000):
            for mi in (0, 1, 3, 6, 20, 21, 100):
                for mx in (-3, 0, 1, 5, 300, 100000):
                    par, plan = N.Sim3Params(), N.Sim3Plan()
                    par.probability, par.min_inliers, par.max_iterations = prob, mi, mx
                    assert lib.hs_sim3_plan(N_, C.byref(par), C.byref(plan)) == N.HS_OK
                    its, eps = R.plan(N_, prob, mi, mx)
                    assert plan.max_iterations == its, (prob, N_, mi, mx, plan.max_iterations, its)
                    assert np.float32(plan.epsilon) == eps or (plan.epsilon != plan.epsilon and eps != eps), (N_, mi)
                    n += 1
    assert n == 8 * 12 * 7 * 6
    par, plan = N.Sim3Params(), N.Sim3Plan()
    par.probability, par.min_inliers, par.max_iterations = 0.99, 20, 300
    assert lib.hs_sim3_plan(100, C.byref(par), C.byref(plan)) == N.HS_OK and (plan.max_iterations, np.float32(plan.epsilon)) == (300, np.float32(0.2))
    assert lib.hs_sim3_plan(-1, C.byref(par), C.byref(plan)) == N.HS_ERR_INVALID and lib.hs_sim3_plan(100, None, C.byref(plan)) == N.HS_ERR_INVALID


def test_work_bytes_equal_the_carve():
    """the carve of hs_sim3.h: 16 floats per hypothesis rounded to 256, a count per hypothesis rounded to 256, 256 spare bytes"""
    from hyslam_amd import _native as N
    lib = N.lib()
    up = lambda v: (v + 255) & ~255
    last = 0
    for Q, n, H in ((0, 0, 0), (1, 0, 1), (1, 9, 1), (1, 65, 12), (3, 86, 12), (8, 4000, 300), (17, 8000, 300)):
        got = int(lib.hs_sim3_work_bytes(Q, n, H))
        assert got == up(Q * H * 64) + up(Q * H * 4) + 256 and got >= last, (Q, n, H, got)
        last = got
    assert lib.hs_sim3_work_bytes(-1, -1, -1) == lib.hs_sim3_work_bytes(0, 0, 0) == 256


def test_refusals_that_need_no_handle():
    from hyslam_amd import _native as N
    lib = N.lib()
    assert lib.hs_sim3_iterate(None, 1, *[None] * 3, 5, None, 0, *[None] * 4) == N.HS_ERR_INVALID
    assert lib.hs_sim3_iterate_device(None, 1, *[None] * 3, 5, None, 0, *[None] * 6) == N.HS_ERR_INVALID
    st = N.Sim3State(7, 7)
    st.s = 3.0
    lib.hs_sim3_state_init(C.byref(st))
    lib.hs_sim3_state_init(None)
    assert (st.iterations, st.best_inliers, st.s, list(st.T12), list(st.R)) == (0, 0, 0.0, [0.0] * 16, [0.0] * 9)


needs_hipcc = pytest.mark.skipif((shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc")) or not os.path.exists(os.path.join(SAN, "..", "host_sanitize", "Makefile")),
                                 reason="needs hipcc (host-only compile) and tests/cpp/host_sanitize/, whose objects it links")


@needs_hipcc
def test_host_side_under_sanitizers():
    """tests/cpp/sim3_sanitize: a stand-alone program, ASan + UBSan, CPU only"""
    subprocess.check_call(["make", "-s", "-j4", "-C", SAN], timeout=1500)
    r = subprocess.run([os.path.join(SAN, "_build", "sim3_sanitize")], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "SIM3 SANITIZE OK" in r.stdout, out[-4000:]
    assert "refusals: 37 refused calls enqueued nothing" in r.stdout and "plan: 1960 parameter sets" in r.stdout and "layout: 80 carves" in r.stdout, out[-4000:]
    assert not any(x in out for x in ("ERROR: AddressSanitizer", "runtime error", "ERROR: LeakSanitizer")), out[-4000:]


@needs_hipcc
def test_kernel_math_on_the_host_equals_the_reference(tmp_path):
    """tests/cpp/sim3_sanitize/sim3_host_math: sim3_sample, sim3_solve, sim3_transforms, sim3_record, sim3_inlier and sim3_walk of kernels_sim3.hip — the
    source the kernels run — compiled for the host, against tests/ref_sim3.py: the samples, every mask and count, R, t, s and both transforms of every
    hypothesis float for float (NaN equal to NaN), and the walk over the counts"""
    import struct

    import ref_sim3 as R
    import sim3_cases as SC
    subprocess.check_call(["make", "-s", "-j4", "-C", SAN], timeout=1500)
    poses = 0
    for name, n_hyp in (("n100", 12), ("n100_sparse", 70), ("n40_fix_scale", 10), ("n30_same_camera", 12), ("n257", 5), ("identical_sets", 3), ("z_zero_or_negative", 6),
                        ("n3_min2", 4)):
        c = SC.cases()[name]
        s = R.Solver(c["corrs"], c["k1"], c["k2"], c["params"], None)     # the generator alone: the program takes no table
        path = str(tmp_path / (name + ".bin"))
        with open(path, "wb") as f:
            f.write(struct.pack("<iiiiQ8f", s.N, n_hyp, c["params"]["fix_scale"], c["params"]["min_inliers"], c["params"]["seed"], *[float(x) for x in c["k1"]],
                                *[float(x) for x in c["k2"]]))
            f.write(np.ascontiguousarray(c["corrs"]).tobytes())
        r = subprocess.run([os.path.join(SAN, "_build", "sim3_host_math"), path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (name, r.stderr[-2000:])
        smp, Rm, t, sc, a, b, masks = s.hypotheses(0, n_hyp)
        for ln in r.stdout.strip().split("\n"):
            w = ln.split()
            it = int(w[1])
            if w[0] == "S":
                assert [int(x) for x in w[2:]] == smp[it], (name, it, "sample")
            elif w[0] == "M":
                assert [int(ch) for ch in w[2]] == masks[it].astype(int).tolist(), (name, it, "mask")
            elif w[0] == "H":
                got = np.array([float.fromhex(x) for x in w[3:]], np.float32)
                want = np.concatenate([Rm[it].reshape(-1), t[it], [sc[it]], a[it].reshape(-1), b[it].reshape(-1)]).astype(np.float32)
                assert int(w[2]) == int(masks[it].sum()) and np.array_equal(got, want, equal_nan=True), (name, it, "pose")
                poses += 1
            else:
                found, rec, best = R.loop_form([int(m.sum()) for m in masks], 0, c["params"]["min_inliers"])
                assert [int(x) for x in w[1:]] == [-1 if found is None else found, -1 if rec is None else rec, best], (name, "walk")
    assert poses == 122


@needs_hipcc
def test_sampler_over_every_randi_sequence_equals_the_reference(tmp_path):
    """sim3_host_math --samples with a directed table: every sequence of randi for n = 3 .. 7 (at most 7 * 6 * 5 samples per n), each printed sample
    against sample() of tests/ref_sim3.py on the same words.  The enumeration holds the samples on which the write by VALUE (Sim3Solver.cc:167-181)
    and the write at the place randi (PnPsolver.cc:194-207) give different results — a draw that hits a place an earlier draw of the same sample
    modified — counted from the two references, which is where a sampler shared by both solvers can be merged wrongly."""
    import struct

    import ref_pnp
    import ref_sim3 as R
    from ransac_enum import randi_table
    subprocess.check_call(["make", "-s", "-j4", "-C", SAN], timeout=1500)
    diverging = checked = 0
    for n in (3, 4, 5, 6, 7):
        table = randi_table(n, 3, R.DRAW_STRIDE)
        want = [R.sample(n, row) for row in table]
        diverging += sum(w != ref_pnp.sample(n, 3, row) for w, row in zip(want, table))
        path, dpath = str(tmp_path / ("enum%d.bin" % n)), str(tmp_path / ("enum%d.draws" % n))
        with open(path, "wb") as f:
            f.write(struct.pack("<iiiiQ8f", n, len(table), 1, 0, 0, *[1.0] * 8))
            f.write(np.zeros(n, R.CORR_DTYPE).tobytes())
        table.tofile(dpath)
        r = subprocess.run([os.path.join(SAN, "_build", "sim3_host_math"), path, dpath, "--samples"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (n, r.stderr[-2000:])
        lines = [ln.split() for ln in r.stdout.strip().split("\n")]
        assert [w[0] for w in lines] == ["S"] * len(table) and [int(w[1]) for w in lines] == list(range(len(table))), n
        for w, s in zip(lines, want):
            assert [int(x) for x in w[2:]] == s, (n, w, s)
            checked += 1
    assert checked == 6 + 24 + 60 + 120 + 210 and diverging > 0
