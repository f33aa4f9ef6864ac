#!/usr/bin/env python3
"""What the batched Horn Sim3 RANSAC costs (hs_sim3_iterate_device).  No threshold: nothing here is a pass criterion, and the parent
commit has no device form to compare with.

For Q = 1 and Q = 8 candidates of N = 100 correspondences (85 % gross outliers, so that no hypothesis returns early and a call runs its whole range),
with n = 5 iterations (one round of LoopClosing::ComputeSim3) and n = 300 (the plan's cap), two ways:

  device     hs_sim3_iterate_device on resident buffers, ONE call for all Q candidates.  Timed on the host clock around `iters` calls that end in one
             stream synchronise; every call is preceded on the stream by a device-to-device copy that puts the fresh states back (a call continues a
             problem otherwise), which is inside the figure.  Median of `repeats` batches, smallest and largest beside it.
  host math  tests/cpp/bench_sim3_host.cpp: the same __host__ __device__ source the kernels run (sample, ComputeSim3, transforms, inlier count, walk,
             mask), compiled for the host, one core, one candidate after another

usage: bench_sim3.py [--iters 50] [--repeats 5]"""
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


def build_host_math():
    src = os.path.join(ROOT, "tests", "cpp", "bench_sim3_host.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "bench_sim3_host")
    deps = [src, os.path.join(ROOT, "hyslam_amd", "csrc", "kernels_sim3.hip"), os.path.join(ROOT, "hyslam_amd", "csrc", "hs_sim3.h"),
            os.path.join(ROOT, "hyslam_amd", "csrc", "hs_ransac.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                               "-I" + os.path.join(ROOT, "hyslam_amd", "csrc"), src, "-o", exe])
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import hipmem
    import hyslam_amd as HS
    import sim3_cases as SC
    from hyslam_amd import _native as N
    exe = build_host_math()
    ex = HS.ORBExtractor(device=0)
    lib = ex._lib
    stream = hipmem.Stream(non_blocking=True)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    rows, n = [], 100
    for Q in (1, 8):
        for H in (5, 300):
            par = np.zeros(Q, N.SIM3_PARAMS_DTYPE)
            par["probability"], par["min_inliers"], par["max_iterations"] = 0.99, 20, 300
            par["fx1"], par["fy1"], par["cx1"], par["cy1"] = SC.K1
            par["fx2"], par["fy2"], par["cx2"], par["cy2"] = SC.K2
            par["seed"] = 100 + np.arange(Q)
            off = np.arange(Q + 1, dtype=np.int64) * n
            corrs = np.concatenate([SC.scene(500 + q, n, 0.85) for q in range(Q)]).view(N.SIM3_CORR_DTYPE)
            D = hipmem.DevBuf
            sb = Q * N.SIM3_STATE_DTYPE.itemsize
            d_corrs, d_fresh, d_states = D.from_numpy(corrs), D.from_numpy(np.zeros(Q, N.SIM3_STATE_DTYPE)), D(sb)
            d_best, d_inl, d_res = D(Q * n), D(Q * n), D(Q * N.SIM3_RESULT_DTYPE.itemsize)
            d_work = D(lib.hs_sim3_work_bytes(Q, Q * n, H))

            def call():
                hipmem.copy_async(d_states.ptr, d_fresh.ptr, sb, stream)
                N.check(ex._h, lib.hs_sim3_iterate_device(ex._h, Q, p(par), p(off), d_corrs.ptr, H, None, 0, d_states.ptr, d_best.ptr, d_res.ptr, d_inl.ptr, d_work.ptr,
                                                          stream.ptr))

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
            res = d_res.to_numpy(N.SIM3_RESULT_DTYPE, Q)
            row = dict(Q=Q, N=n, n_iterations=H, device_us=round(float(np.median(batches)), 1), device_min_max_us=[round(min(batches), 1), round(max(batches), 1)],
                       status=[int(s) for s in res["status"]], hypotheses_run=[int(s) for s in res["hypotheses_run"]])
            case = os.path.join(os.path.dirname(exe), "bench_sim3_case.bin")
            with open(case, "wb") as f:
                f.write(np.array([Q, n, H], np.int32).tobytes() + par.tobytes() + corrs.tobytes())
            out = subprocess.run([exe, case, str(max(5, a.iters // 5))], capture_output=True, text=True, check=True).stdout.split()
            row["host_math_one_core_us"] = float(out[0])
            rows.append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps(dict(iters=a.iters, repeats=a.repeats, rows=rows)))


if __name__ == "__main__":
    main()
