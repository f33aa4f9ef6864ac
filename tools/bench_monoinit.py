#!/usr/bin/env python3
"""Times the monocular initialisation (hs_monoinit_estimate_device) on one device: milliseconds per call for Q = 1 and 2 problems of
N = 500 and 2000 matches at 200 iterations, for BOTH layouts of stage 2 (hs_debug_monoinit_layout: 0 = one wave per hypothesis and model, 1 = one
lane per hypothesis), beside a single-thread host build of the same __host__ __device__ math
(tests/cpp/monoinit_sanitize/monoinit_host_math.cpp, compiled here without sanitizers at -O2).  No target is fixed in advance: the GPU figure is
reported against that host build.  Device: resident buffers, ONE call for all Q problems, host clock around `calls` calls that end in one stream
synchronise; every call is checked to give the same result bytes in both layouts.  Prints one JSON line per configuration.

    python tools/bench_monoinit.py [--calls 20] [--repeats 5] [--host-repeat 3] [--no-host]
"""
import argparse
import ctypes as C
import json
import os
import re
import struct
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HOST_SRC = os.path.join(ROOT, "tests", "cpp", "monoinit_sanitize", "monoinit_host_math.cpp")
HOST_DIR = os.path.join(ROOT, "tools", "_build_monoinit")
HOST_EXE = os.path.join(HOST_DIR, "monoinit_host_math")
CAM = (500.0, 500.0, 320.0, 240.0)


def scene(seed, N):
    """a general two-view scene of N matches (depths 3 .. 9, 0.3 px noise, 10 % gross outliers) among n1 = 3 N / 2 and n2 = 3 N / 2 + 7 key points"""
    from hyslam_amd.synth import splitmix64
    u01 = lambda n, s: (splitmix64(seed, n, s) >> np.uint64(11)).astype(np.float64) / float(1 << 53)
    u, v, z = u01(N, 1) - 0.5, (u01(N, 2) - 0.5) * 0.75, 3.0 + 6.0 * u01(N, 3)
    X = np.stack([u * z, v * z, z], 1)
    a = 0.05
    Rm = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    X2 = X @ Rm.T + np.array([0.4, 0.05, 0.1])
    proj = lambda P: np.stack([CAM[0] * P[:, 0] / P[:, 2] + CAM[2], CAM[1] * P[:, 1] / P[:, 2] + CAM[3]], 1)
    p1 = proj(X) + (np.stack([u01(N, 4), u01(N, 5)], 1) - 0.5) * 0.6
    p2 = proj(X2) + (np.stack([u01(N, 6), u01(N, 7)], 1) - 0.5) * 0.6
    out = u01(N, 8) < 0.1
    p2[out] = np.stack([u01(N, 9) * 640, u01(N, 10) * 480], 1)[out]
    n1, n2 = N + N // 2, N + N // 2 + 7
    k1, k2 = np.stack([u01(n1, 11) * 640, u01(n1, 12) * 480], 1), np.stack([u01(n2, 13) * 640, u01(n2, 14) * 480], 1)
    place1, place2 = np.sort(np.argsort(u01(n1, 15), kind="stable")[:N]), np.argsort(u01(n2, 16), kind="stable")[:N]
    k1[place1], k2[place2] = p1, p2
    m = np.full(n1, -1, np.int32)
    m[place1] = place2
    return k1.astype(np.float32), k2.astype(np.float32), m


def host_ms(k1, k2, m, par, repeat):
    if not os.path.exists(HOST_EXE):
        os.makedirs(HOST_DIR, exist_ok=True)
        hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
        subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-w",
                               "-I" + os.path.join(ROOT, "hyslam_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), HOST_SRC, "-o", HOST_EXE,
                               "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    src, dst = os.path.join(HOST_DIR, "in.bin"), os.path.join(HOST_DIR, "out.bin")
    with open(src, "wb") as f:
        f.write(par.tobytes())
        f.write(struct.pack("<4i", len(k1), len(k2), 0, 0))
        f.write(k1.tobytes() + k2.tobytes() + m.tobytes())
    out = subprocess.run([HOST_EXE, src, dst, "--repeat", str(repeat)], capture_output=True, text=True, check=True).stdout
    return float(re.search(r"ms=([0-9.]+)", out).group(1)), int(re.search(r"status=(\d+)", out).group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeat", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import hyslam_amd as HS
    from hyslam_amd import _native as N
    from hyslam_amd.features import _DevBuf
    ex = HS.ORBExtractor(device=0)
    lib = ex._lib
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    for n_matches in (500, 2000):
        for Q in (1, 2):
            scenes = [scene(100 + q, n_matches) for q in range(Q)]
            par = np.zeros(Q, N.MONOINIT_PARAMS_DTYPE)
            par["fx"], par["fy"], par["cx"], par["cy"] = CAM
            par["sigma"], par["max_iterations"], par["min_triangulated"], par["min_frac_triangulated"], par["min_parallax_deg"] = 1.0, 200, 50, 0.9, 1.0
            par["seed"] = np.arange(Q) + 7

            def kp(xy):
                k = np.zeros(len(xy), N.KP_DTYPE)
                k["x"], k["y"] = xy[:, 0], xy[:, 1]
                return k
            k1, k2 = np.concatenate([kp(s[0]) for s in scenes]), np.concatenate([kp(s[1]) for s in scenes])
            m = np.concatenate([s[2] for s in scenes])
            off1, off2 = np.zeros(Q + 1, np.int64), np.zeros(Q + 1, np.int64)
            off1[1:], off2[1:] = np.cumsum([len(s[0]) for s in scenes]), np.cumsum([len(s[1]) for s in scenes])
            n1 = len(k1)
            nwork = int(lib.hs_monoinit_work_bytes(Q, n1, 200))
            d_k1, d_k2, d_m = _DevBuf(ex, k1.nbytes, k1), _DevBuf(ex, k2.nbytes, k2), _DevBuf(ex, m.nbytes, m)
            d_res, d_ih, d_if = _DevBuf(ex, Q * N.MONOINIT_RESULT_DTYPE.itemsize), _DevBuf(ex, n1), _DevBuf(ex, n1)
            d_p3d, d_tri, d_work = _DevBuf(ex, 12 * n1), _DevBuf(ex, n1), _DevBuf(ex, nwork)

            def call():
                N.check(ex._h, lib.hs_monoinit_estimate_device(ex._h, Q, p(par), p(off1), d_k1.ptr, p(off2), d_k2.ptr, d_m.ptr, None, 0, d_res.ptr, d_ih.ptr, d_if.ptr,
                                                               d_p3d.ptr, d_tri.ptr, d_work.ptr, None))
            ms, bytes_of = {}, {}
            try:
                for layout in (0, 1):
                    lib.hs_debug_monoinit_layout(layout)
                    call()
                    ex.synchronize()
                    bytes_of[layout] = d_res.read(np.uint8, Q * N.MONOINIT_RESULT_DTYPE.itemsize).tobytes() + d_p3d.read(np.uint8, 12 * n1).tobytes()
                    best = 1e30
                    for _ in range(args.repeats):
                        t0 = time.perf_counter()
                        for _ in range(args.calls):
                            call()
                        ex.synchronize()
                        best = min(best, (time.perf_counter() - t0) * 1e3 / args.calls)
                    ms[layout] = best
            finally:
                lib.hs_debug_monoinit_layout(0)
            res = np.frombuffer(bytes_of[0][:Q * N.MONOINIT_RESULT_DTYPE.itemsize], N.MONOINIT_RESULT_DTYPE)
            line = dict(N=n_matches, Q=Q, iterations=200, n1=int(off1[1]), n2=int(off2[1]), status=[int(s) for s in res["status"]],
                        ms_per_call_wave_per_hypothesis=round(ms[0], 4), ms_per_call_lane_per_hypothesis=round(ms[1], 4), same_bytes=bytes_of[0] == bytes_of[1])
            if not args.no_host:
                hm = [host_ms(scenes[q][0], scenes[q][1], scenes[q][2], par[q:q + 1], args.host_repeat) for q in range(Q)]
                line["host_single_thread_ms"] = round(sum(h[0] for h in hm), 3)
                line["host_status"] = [h[1] for h in hm]
                line["speedup_vs_host_wave"] = round(line["host_single_thread_ms"] / ms[0], 1)
                line["speedup_vs_host_lane"] = round(line["host_single_thread_ms"] / ms[1], 1)
            print(json.dumps(line), flush=True)
            for b in (d_k1, d_k2, d_m, d_res, d_ih, d_if, d_p3d, d_tri, d_work):
                b.free()


if __name__ == "__main__":
    main()
