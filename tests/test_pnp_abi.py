"""The batched EPnP RANSAC (include/hyslam_amd.h: hs_pnp_*), what can be checked without a GPU: the ctypes structs and numpy dtypes of
hyslam_amd/_native.py against sizeof / offsetof of the header itself (a C program compiled here), the status values, the work area's size, the
refusals that need no handle, and the host side under ASan + UBSan as a stand-alone program (tests/cpp/pnp_sanitize/: hs_pnp_plan, "a refused call
enqueues nothing" for both forms on a stub runtime, the carve of the work area; nothing is loaded into python), and the kernels' own math —
kernels_pnp.hip compiled for the host, tests/cpp/pnp_sanitize/pnp_host_math.cpp — against LITERAL of tests/ref_pnp.py bit for bit."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SAN = os.path.join(ROOT, "tests", "cpp", "pnp_sanitize")

STRUCTS = {
    "hs_pnp_corr": ("PnpCorr", "PNP_CORR_DTYPE", ("Xw", "u", "v", "sigma2", "kp", "_pad")),
    "hs_pnp_params": ("PnpParams", "PNP_PARAMS_DTYPE", ("probability", "min_inliers", "max_iterations", "min_set", "epsilon", "th2", "fx", "fy", "cx", "cy", "_pad", "seed")),
    "hs_pnp_plan_t": ("PnpPlan", None, ("min_inliers", "epsilon", "max_iterations", "_pad")),
    "hs_pnp_state": ("PnpState", "PNP_STATE_DTYPE", ("iterations", "best_inliers", "best_Tcw")),
    "hs_pnp_result": ("PnpResult", "PNP_RESULT_DTYPE", ("Tcw_d", "Tcw", "status", "n_inliers", "at_iteration", "iterations", "hypotheses_run", "refines_run")),
}
STATUS = ("HS_PNP_TOO_FEW", "HS_PNP_REFINED", "HS_PNP_BEST", "HS_PNP_NONE", "HS_PNP_NONFINITE", "HS_PNP_MAX_SET")


def header_layout():
    """{struct: (sizeof, {field: offsetof})} and {constant: value}, as a C compiler reads include/hyslam_amd.h"""
    os.makedirs(BUILD, exist_ok=True)
    src, exe = os.path.join(BUILD, "pnp_layout.c"), os.path.join(BUILD, "pnp_layout")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "hyslam_amd.h"', "int main(void) {"]
    for s, (_, _, fields) in STRUCTS.items():
        lines.append('printf("S %s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['printf("F %s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f) for f in fields]
    lines += ['printf("K %s %%d\\n", (int)%s);' % (k, k) for k in STATUS]
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
    assert (sizes["hs_pnp_corr"], sizes["hs_pnp_params"], sizes["hs_pnp_plan_t"], sizes["hs_pnp_state"], sizes["hs_pnp_result"]) == (32, 56, 16, 72, 216)
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
    assert [consts[k] for k in STATUS] == [N.HS_PNP_TOO_FEW, N.HS_PNP_REFINED, N.HS_PNP_BEST, N.HS_PNP_NONE, N.HS_PNP_NONFINITE, N.HS_PNP_MAX_SET] == [0, 1, 2, 3, 4, 16]
    import ref_pnp as R
    assert R.CORR_DTYPE == N.PNP_CORR_DTYPE and (R.TOO_FEW, R.REFINED, R.BEST, R.NONE, R.NONFINITE, R.MAX_SET) == (0, 1, 2, 3, 4, 16)


def test_work_bytes_hold_their_parts_and_never_decrease():
    from hyslam_amd import _native as N
    lib = N.lib()
    last = 0
    for Q, n, H in ((0, 0, 0), (1, 0, 1), (1, 9, 1), (1, 65, 12), (3, 86, 12), (8, 4000, 300), (16, 8000, 300)):
        got = int(lib.hs_pnp_work_bytes(Q, n, H))
        assert got >= Q * H * (12 * 8 + 4) + n * (5 * 8 + 1) and got >= last and got % 256 == 0, (Q, n, H, got)
        last = got
    assert lib.hs_pnp_work_bytes(-1, -1, -1) == lib.hs_pnp_work_bytes(0, 0, 0)


def test_refusals_that_need_no_handle():
    """the argument checks run before anything is enqueued; with a handle they are held to that by tests/cpp/pnp_sanitize (below) and on the device by
    tests/test_gpu_pnp.py"""
    from hyslam_amd import _native as N
    lib = N.lib()
    assert lib.hs_pnp_iterate(*[None] * 1, 1, *[None] * 3, 5, None, 0, *[None] * 4) == N.HS_ERR_INVALID
    assert lib.hs_pnp_iterate_device(None, 1, *[None] * 3, 5, None, 0, *[None] * 6) == N.HS_ERR_INVALID
    st = N.PnpState(7, 7)
    lib.hs_pnp_state_init(C.byref(st))
    lib.hs_pnp_state_init(None)
    assert (st.iterations, st.best_inliers, list(st.best_Tcw)) == (0, 0, [0.0] * 16)


@pytest.mark.skipif((shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc")) or not os.path.exists(os.path.join(SAN, "..", "host_sanitize", "Makefile")),
                    reason="needs hipcc (host-only compile) and tests/cpp/host_sanitize/, whose objects it links")
def test_host_side_under_sanitizers():
    """tests/cpp/pnp_sanitize: a stand-alone program, ASan + UBSan, CPU only"""
    subprocess.check_call(["make", "-s", "-j4", "-C", SAN], timeout=1500)
    r = subprocess.run([os.path.join(SAN, "_build", "pnp_sanitize")], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "PNP SANITIZE OK" in r.stdout, out[-4000:]
    assert "refusals: 35 refused calls enqueued nothing" in r.stdout and "plan: 11200 parameter sets" in r.stdout, out[-4000:]
    assert not any(x in out for x in ("ERROR: AddressSanitizer", "runtime error", "ERROR: LeakSanitizer")), out[-4000:]


@pytest.mark.skipif((shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc")) or not os.path.exists(os.path.join(SAN, "..", "host_sanitize", "Makefile")),
                    reason="needs hipcc (host-only compile) and tests/cpp/host_sanitize/, whose objects it links")
def test_kernel_math_on_the_host_equals_literal(tmp_path):
    """tests/cpp/pnp_sanitize/pnp_host_math: pnp_sample, pnp_epnp and pnp_inlier of kernels_pnp.hip — the source the kernels run — compiled for the host,
    against LITERAL of tests/ref_pnp.py: the samples, every count, and the twelve doubles of every hypothesis and of every refine, bit for bit"""
    import struct

    import numpy as np

    import pnp_cases as PC
    import ref_pnp as R
    subprocess.check_call(["make", "-s", "-j4", "-C", SAN], timeout=1500)
    poses = refines = 0
    for name, n_hyp in (("n12", 6), ("n64", 8), ("n65", 4), ("n300", 12), ("nonfinite_corr", 3)):
        c = PC.cases()[name]
        s = R.Solver(c["corrs"], c["cam"], c["params"], None)         # the generator alone: the program takes no table
        path = str(tmp_path / (name + ".bin"))
        with open(path, "wb") as f:
            f.write(struct.pack("<iiiiQ5f", s.N, c["params"]["min_set"], n_hyp, s.min_inliers, c["params"]["seed"], c["params"]["th2"], *[float(x) for x in c["cam"]]))
            f.write(np.ascontiguousarray(c["corrs"]).tobytes())
        r = subprocess.run([os.path.join(SAN, "_build", "pnp_host_math"), path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (name, r.stderr[-2000:])
        for ln in r.stdout.strip().split("\n"):
            w = ln.split()
            it = int(w[1])
            cnt, best = s.hypothesis(it)
            if w[0] == "S":
                assert [int(x) for x in w[2:]] == best[4], (name, it, "sample")
                continue
            got = np.array([float.fromhex(x) for x in w[3:]])
            if w[0] == "H":
                want_cnt, Rm, t = cnt, best[1], best[2]
                poses += 1
            else:
                _, (Rm, t, _, want_cnt) = s.refine(best)
                refines += 1
            assert int(w[2]) == want_cnt, (name, ln[:40])
            assert np.array_equal(got, np.concatenate([Rm.reshape(-1), t]), equal_nan=True), (name, w[0], it, float(np.nanmax(np.abs(got - np.concatenate([Rm.reshape(-1), t])))))
    assert poses == 33 and refines >= 4


@pytest.mark.skipif((shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc")) or not os.path.exists(os.path.join(SAN, "..", "host_sanitize", "Makefile")),
                    reason="needs hipcc (host-only compile) and tests/cpp/host_sanitize/, whose objects it links")
def test_sampler_over_every_randi_sequence_equals_the_reference(tmp_path):
    """pnp_host_math --samples with a directed table: every sequence of randi for n = 4 .. 7 with min_set 4 and n = 5, 6 with min_set 5, each printed
    sample against sample() of tests/ref_pnp.py on the same words.  The enumeration holds the samples on which the write at the place randi
    (PnPsolver.cc:194-207) and the write by VALUE (Sim3Solver.cc:167-181) give different results — a draw that hits a place an earlier draw of the
    same sample modified — counted from the two references over the first three draws, the set the Sim3 reference takes."""
    import struct

    import numpy as np

    import ref_pnp as R
    import ref_sim3
    from ransac_enum import randi_table
    subprocess.check_call(["make", "-s", "-j4", "-C", SAN], timeout=1500)
    diverging = checked = 0
    for n, ms in ((4, 4), (5, 4), (6, 4), (7, 4), (5, 5), (6, 5)):
        table = randi_table(n, ms, R.MAX_SET)
        want = [R.sample(n, ms, row) for row in table]
        diverging += sum(w[:3] != ref_sim3.sample(n, row) for w, row in zip(want, table))
        path, dpath = str(tmp_path / ("enum%d_%d.bin" % (n, ms))), str(tmp_path / ("enum%d_%d.draws" % (n, ms)))
        with open(path, "wb") as f:
            f.write(struct.pack("<iiiiQ5f", n, ms, len(table), ms, 0, *[1.0] * 5))
            f.write(np.zeros(n, R.CORR_DTYPE).tobytes())
        table.tofile(dpath)
        r = subprocess.run([os.path.join(SAN, "_build", "pnp_host_math"), path, dpath, "--samples"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (n, ms, r.stderr[-2000:])
        lines = [ln.split() for ln in r.stdout.strip().split("\n")]
        assert [w[0] for w in lines] == ["S"] * len(table) and [int(w[1]) for w in lines] == list(range(len(table))), (n, ms)
        for w, s in zip(lines, want):
            assert [int(x) for x in w[2:]] == s, (n, ms, w, s)
            checked += 1
    assert checked == 24 + 120 + 360 + 840 + 120 + 720 and diverging > 0
