#!/usr/bin/env python3
"""What the batched EPnP RANSAC costs (hs_pnp_iterate_device).  No threshold: nothing here is a pass criterion, and the parent commit
has no device form to compare with.

For Q = 1 and Q = 8 candidates of N = 100 and N = 500 correspondences (30 % gross outliers, 0.1 px pixel noise), with 35 hypotheses (the plan of the
reference's own parameters) and 300 (its cap), three ways:

  device    hs_pnp_iterate_device on resident buffers, ONE call for all Q candidates.  Timed on the host clock around `iters` calls that end in one
            stream synchronise; every call is preceded on the stream by a device-to-device copy that puts the fresh states back (a call continues a
            problem otherwise), which is inside the figure.  Median of `repeats` batches, smallest and largest beside it.
  host loop tests/cpp/bench_pnp_host.cpp: hs_pnp_iterate (host pointers, staged, synchronous) once per candidate, one after another — a C++ caller
            that keeps the reference's structure
  numpy     the INDEPENDENT reference of tests/ref_pnp.py (numpy.linalg EPnP per hypothesis, a vectorised inlier count, the records form), one
            candidate after another, on the host

A call runs every hypothesis of its range whether or not an earlier one returns, so `hypotheses` is the work of the first kernel; the refines a call
runs depend on the data and are printed.  usage: bench_pnp.py [--iters 50] [--repeats 5] [--no-numpy]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def numpy_reference(R, corrs, cam, params, H):
    """INDEPENDENT over one candidate: H hypotheses, then the records walk with Refine() once per record.  Returns the status."""
    fu, fv, uc, vc = [float(c) for c in cam]
    X, uv, lim = corrs["Xw"].astype(np.float64), np.stack([corrs["u"], corrs["v"]], 1).astype(np.float64), corrs["sigma2"] * np.float32(params["th2"])
    n_min = R.plan(len(corrs), **params)[0]

    def count(Rm, t):
        with np.errstate(all="ignore"):
            Pc = X @ Rm.T + t
            e = (uv[:, 0] - (uc + fu * Pc[:, 0] / Pc[:, 2])) ** 2 + (uv[:, 1] - (vc + fv * Pc[:, 1] / Pc[:, 2])) ** 2
        return e < lim

    best, status = 0, R.NONE
    for it in range(H):
        idx = R.sample(len(corrs), 4, [R.draw32(params["seed"], it, k, 4) for k in range(4)])
        mask = count(*R.epnp_independent(R.points_of(corrs, idx), cam))
        if mask.sum() >= n_min and mask.sum() > best:
            best = int(mask.sum())
            if count(*R.epnp_independent(R.points_of(corrs, np.nonzero(mask)[0]), cam)).sum() > n_min:
                return R.REFINED
            status = R.BEST
    return status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    import hipmem
    import hyslam_amd as HS
    import pnp_cases as PC
    import ref_pnp as R
    from hyslam_amd import _native as N
    ex = HS.ORBExtractor(device=0)
    lib = ex._lib
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "bench_pnp_host")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "bench_pnp_host.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "hyslam_amd"),
                           "-lhyslam_amd", "-Wl,-rpath," + os.path.join(ROOT, "hyslam_amd")])
    stream = hipmem.Stream(non_blocking=True)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    rows = []
    for Q in (1, 8):
        for n in (100, 500):
            for H in (35, 300):
                params = dict(R.DEFAULT, max_iterations=H, seed=0)
                scenes = [PC.scene(500 + q, n, 0.3)[0] for q in range(Q)]
                par = np.zeros(Q, N.PNP_PARAMS_DTYPE)
                for q in range(Q):
                    for k in ("probability", "min_inliers", "max_iterations", "min_set", "epsilon", "th2"):
                        par[k][q] = params[k]
                    par["fx"][q], par["fy"][q], par["cx"][q], par["cy"][q] = PC.CAM
                    par["seed"][q] = 100 + q
                off = np.arange(Q + 1, dtype=np.int64) * n
                corrs = np.concatenate(scenes).view(N.PNP_CORR_DTYPE)
                D = hipmem.DevBuf
                d_corrs, d_fresh, d_states = D.from_numpy(corrs), D.from_numpy(np.zeros(Q, N.PNP_STATE_DTYPE)), D(Q * N.PNP_STATE_DTYPE.itemsize)
                d_best, d_inl, d_res = D(Q * n), D(Q * n), D(Q * N.PNP_RESULT_DTYPE.itemsize)
                d_work = D(lib.hs_pnp_work_bytes(Q, Q * n, H))

                def call():
                    hipmem.copy_async(d_states.ptr, d_fresh.ptr, Q * N.PNP_STATE_DTYPE.itemsize, stream)
                    N.check(ex._h, lib.hs_pnp_iterate_device(ex._h, Q, p(par), p(off), d_corrs.ptr, H, None, 0, d_states.ptr, d_best.ptr, d_res.ptr, d_inl.ptr,
                                                             d_work.ptr, stream.ptr))

                for _ in range(3):
                    call()
                stream.synchronize()
                batches = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    for _ in range(a.iters):
                        call()
                    stream.synchronize()
                    batches.append((time.perf_counter() - t0) * 1e6 / a.iters)
                res = d_res.to_numpy(N.PNP_RESULT_DTYPE, Q)
                row = dict(Q=Q, N=n, hypotheses=H, device_us=round(float(np.median(batches)), 1), device_min_max_us=[round(min(batches), 1), round(max(batches), 1)],
                           status=[int(s) for s in res["status"]], refines=[int(s) for s in res["refines_run"]], at_iteration=[int(s) for s in res["at_iteration"]])
                case = os.path.join(os.path.dirname(exe), "bench_pnp_case.bin")
                with open(case, "wb") as f:
                    f.write(np.array([Q, n, H], np.int32).tobytes() + par.tobytes() + corrs.tobytes())
                out = subprocess.run([exe, case, str(max(5, a.iters // 5))], capture_output=True, text=True, check=True).stdout.split()
                row["host_loop_us"] = float(out[0])
                if not a.no_numpy:
                    t0 = time.perf_counter()
                    st = [numpy_reference(R, scenes[q], PC.CAM, dict(params, seed=100 + q), H) for q in range(Q)]
                    row["numpy_us"], row["numpy_status"] = round((time.perf_counter() - t0) * 1e6, 0), st
                rows.append(row)
                print(json.dumps(row), flush=True)
    print(json.dumps(dict(iters=a.iters, repeats=a.repeats, rows=rows)))


if __name__ == "__main__":
    main()
