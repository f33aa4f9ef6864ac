#!/usr/bin/env python3
"""Times hs_pose_optimize_device (Optimizer::PoseOptimization in one launch, one workgroup per problem) on one MI355X: device time per call at
n = 200, 1000 and 2000 edges per problem, Q = 1, 2 and 64 problems per call, 15 % gross outliers, scenes of tests/poseopt_cases.py.  Reported, not
gated: the feature has no earlier timing to beat; what matters for a resident tracking chain is this time next to hs_local_map_search_device's.

  device_us      HIP events around `--iters` back-to-back calls on one stream, divided by the number of calls; median, smallest and largest of
                 `--repeats` such batches after a warm-up of the same shape.  Launch gaps between the calls are inside.
  numpy_ref_ms   wall time of tests/ref_poseopt.pose_optimization_fast for ONE of the problems on this host's CPU.  This is the project's float64
                 numpy restatement, NOT g2o: nobody has measured g2o on this path, and it cannot be built here.  It is printed to show the order of
                 magnitude of a host round trip's compute, not as a speed-up claim.
  check          n_good of the first problem against the numpy reference (a timing of wrong results is worthless)

--libs label=path,...  times other builds of the same sources as well, each in a process of its own (HYSLAM_AMD_LIB), e.g. the workgroup sizes:
    make -C hyslam_amd/csrc BUILD=_build_po128 OUT=../libhyslam_amd_po128.so EXTRA=-DHS_POSE_THREADS=128
Every measuring process runs under its own time limit and the tool stops at the first one that fails.  Prints one JSON line per build.
usage: bench_pose_optimize.py [--iters 200] [--repeats 7] [--libs po128=hyslam_amd/libhyslam_amd_po128.so] [--step-timeout 240]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES, BATCHES, OUTLIERS = (200, 1000, 2000), (1, 2, 64), 0.15


def scenes(n, Q):
    import poseopt_cases as P
    return [P.scene(5000 + 97 * n + q, n, "mixed", OUTLIERS) for q in range(Q)]


def measure(a):
    """one build (the library HYSLAM_AMD_LIB names, or the product's): every (n, Q)"""
    import torch
    import hyslam_amd as HS
    from hyslam_amd import _native as N
    import ref_poseopt as R
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    ex = HS.ORBExtractor(device=0)
    stream = torch.cuda.Stream()
    rows = []
    for n in SIZES:
        for Q in BATCHES:
            items = scenes(n, Q)
            prob = np.zeros(Q, N.POSE_PROBLEM_DTYPE)
            for q, (T, cam, _) in enumerate(items):
                prob["Tcw"][q] = T.reshape(16)
                for k, v in zip(("fx", "fy", "cx", "cy", "bf"), cam):
                    prob[k][q] = v
            off = np.arange(Q + 1, dtype=np.int64) * n
            d_prob, d_off, d_edges = up(prob), up(off), up(np.concatenate([e for _, _, e in items]))
            d_out = torch.zeros(Q * n, dtype=torch.uint8, device=dev)
            d_res = torch.zeros(Q * N.POSE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            call = lambda: ex.pose_optimize_device(Q, d_prob.data_ptr(), d_edges.data_ptr(), d_out.data_ptr(), d_res.data_ptr(),
                                                   d_edge_offsets=d_off.data_ptr(), stream=stream.cuda_stream)
            for _ in range(20):
                call()
            stream.synchronize()
            us = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.iters):
                    call()
                e1.record(stream)
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / a.iters)
            res = d_res.cpu().numpy().view(N.POSE_RESULT_DTYPE)
            row = dict(n=n, Q=Q, device_us=round(float(np.median(us)), 2), device_us_min=round(min(us), 2), device_us_max=round(max(us), 2),
                       lm_iterations=int(res["lm_iterations"][0]), lm_trials=int(res["lm_trials"][0]), n_good=int(res["n_good"][0]))
            if Q == 1:
                t0 = time.perf_counter()
                ref = R.pose_optimization_fast(*items[0])
                row["numpy_ref_ms_not_g2o"] = round((time.perf_counter() - t0) * 1e3, 2)
                row["check"] = "ok" if ref["n_good"] == row["n_good"] and np.array_equal(ref["outlier"], d_out.cpu().numpy()[:n]) else "DIFFERS"
            rows.append(row)
    print(json.dumps(dict(build=a.label, lib=os.environ.get("HYSLAM_AMD_LIB", "product"), iters=a.iters, repeats=a.repeats, outliers=OUTLIERS, rows=rows)))
    return 0 if all(r.get("check", "ok") == "ok" for r in rows) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--libs", default="", help="label=path,... further builds of the same sources")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each measuring process may take")
    ap.add_argument("--label", default=None, help=argparse.SUPPRESS)            # set for the measuring process itself
    a = ap.parse_args()
    if a.label is not None:
        return measure(a)
    builds = [("product", None)] + [tuple(x.split("=", 1)) for x in a.libs.split(",") if x]
    for label, path in builds:
        env = dict(os.environ)
        if path:
            path = os.path.abspath(path)
            if not os.path.exists(path):
                print("bench_pose_optimize: %s not found" % path)
                return 1
            env["HYSLAM_AMD_LIB"] = path
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--label", label, "--iters", str(a.iters),
               "--repeats", str(a.repeats)]
        rc = subprocess.call(cmd, env=env)
        if rc != 0:                                              # a failure, a fault or the time limit: nothing more is started on the GPU
            print("bench_pose_optimize: build %s ended with status %d; stopping" % (label, rc))
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
