#!/usr/bin/env python3
"""Batched landmark representative descriptors (hs_landmark_best_descriptors*, MapPointDB.cpp:128-175): prints one JSON line.

Per shape (L landmarks, N observations each drawn as named):
  device_us      hs_landmark_best_descriptors_device on a caller stream, data resident in HBM: device-event time per batch (median of the runs)
  host_api_us    hs_landmark_best_descriptors from host memory (upload, kernels, download, synchronise): wall time per batch (median)
  host_baseline_us  a single-thread C++ restatement of the reference's loop (N x N float matrix, std::sort of every row, first strict minimum of
                 the row medians; g++ -O2, compiled by this tool), one landmark after another as hySLAM's mapping thread does: wall time per batch
and landmarks/s for each.  The three must choose the same descriptors (checked; "agree").
Run on the GPU box: python tools/bench_landmark_descriptors.py [--runs R]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hyslam_amd as HS  # noqa: E402

BASELINE_CPP = r"""
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>
// in.bin: int64 L, int64 offsets[L+1], uint8 desc[offsets[L]][32] -> out.bin: int32 best[L]; prints the wall time of the loop in microseconds
static int hamming(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int k = 0; k < 32; k += 8) { uint64_t x, y; __builtin_memcpy(&x, a + k, 8); __builtin_memcpy(&y, b + k, 8); d += __builtin_popcountll(x ^ y); }
    return d;
}
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb"); int64_t L; if (fread(&L, 8, 1, f) != 1) return 2;
    std::vector<int64_t> off(L + 1); if (fread(off.data(), 8, L + 1, f) != (size_t)(L + 1)) return 2;
    std::vector<uint8_t> desc(off[L] * 32); if (off[L] && fread(desc.data(), 32, off[L], f) != (size_t)off[L]) return 2;
    fclose(f);
    std::vector<int32_t> best(L, -1);
    const int reps = argc > 3 ? atoi(argv[3]) : 1;
    const auto t0 = std::chrono::steady_clock::now();
    for (int rep = 0; rep < reps; rep++)
    for (int64_t l = 0; l < L; l++) {
        const size_t N = off[l + 1] - off[l];
        if (N == 0) continue;
        const uint8_t* d = desc.data() + off[l] * 32;
        std::vector<float> D(N * N);
        for (size_t i = 0; i < N; i++) {
            D[i * N + i] = 0;
            for (size_t j = i + 1; j < N; j++) { const float v = (float)hamming(d + i * 32, d + j * 32); D[i * N + j] = v; D[j * N + i] = v; }
        }
        float bestMedian = std::numeric_limits<float>::max(); int bestIdx = 0;
        for (size_t i = 0; i < N; i++) {
            std::vector<int> row(D.begin() + i * N, D.begin() + (i + 1) * N);
            std::sort(row.begin(), row.end());
            const int median = row[(size_t)(0.5 * (N - 1))];
            if (median < bestMedian) { bestMedian = median; bestIdx = (int)i; }
        }
        best[l] = bestIdx;
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
    FILE* o = fopen(argv[2], "wb"); fwrite(best.data(), 4, L, o); fclose(o);
    printf("%.3f\n", us);
    return 0;
}
"""


def make_shape(seed, L, lo, hi, big=0, big_lo=500, big_hi=800):
    rng = np.random.default_rng(seed)
    n = rng.integers(lo, hi + 1, L)
    if big:
        n[rng.choice(L, big, replace=False)] = rng.integers(big_lo, big_hi + 1, big)
    off = np.zeros(L + 1, np.int64)
    np.cumsum(n, out=off[1:])
    # observations of one landmark are views of one point: a few centre descriptors with a few flipped bits
    centre = rng.integers(0, 256, (L, 3, 32), dtype=np.uint8)
    owner = np.repeat(np.arange(L), n)
    desc = centre[owner, rng.integers(0, 3, len(owner))]
    flip = rng.integers(0, 256, (len(owner), 4))
    for k in range(4):
        desc[np.arange(len(owner)), flip[:, k] // 8] ^= (1 << (flip[:, k] % 8)).astype(np.uint8)
    return off, np.ascontiguousarray(desc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    args = ap.parse_args()
    shapes = [
        ("L20000_N2-40_plus20_N500-800", dict(seed=1, L=20000, lo=2, hi=40, big=20)),
        ("L20000_N2-40", dict(seed=2, L=20000, lo=2, hi=40)),
        ("L100000_N2-40", dict(seed=3, L=100000, lo=2, hi=40)),
        ("L2000_N2-12", dict(seed=4, L=2000, lo=2, hi=12)),
        ("L64_N1000", dict(seed=5, L=64, lo=1000, hi=1000)),
    ]
    dev = torch.device("cuda", 0)
    ex = HS.ORBExtractor(device=0)
    fm = HS.FeatureMatcher(extractor=ex)
    ts = torch.cuda.Stream()                      # a real stream handle: 0 would mean "the handle's own stream" to the C ABI
    tmp = tempfile.mkdtemp(prefix="bench_lm_")
    exe = os.path.join(tmp, "baseline")
    with open(exe + ".cpp", "w") as f:
        f.write(BASELINE_CPP)
    subprocess.check_call(["g++", "-O2", "-std=c++17", exe + ".cpp", "-o", exe])
    out = {"tool": "bench_landmark_descriptors", "runs": args.runs, "device": torch.cuda.get_device_name(0),
           "host_baseline": "single-thread C++ restatement of MapPointDB.cpp:128-175 (N x N float matrix, std::sort per row), g++ -O2, one landmark at a time",
           "shapes": {}}
    for name, kw in shapes:
        off, desc = make_shape(**kw)
        L = len(off) - 1
        d_off = torch.from_numpy(off).to(dev); d_desc = torch.from_numpy(desc).to(dev)
        d_best = torch.empty(L, dtype=torch.int32, device=dev); d_med = torch.empty(L, dtype=torch.int32, device=dev)
        run = lambda: ex.landmark_best_descriptors_device(d_off.data_ptr(), L, d_desc.data_ptr(), d_best.data_ptr(), d_med.data_ptr(), stream=ts.cuda_stream)
        torch.cuda.synchronize()
        for _ in range(3):
            run()
        ts.synchronize()
        dt = []
        for _ in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts); run(); e1.record(ts)
            e1.synchronize()
            dt.append(e0.elapsed_time(e1) * 1e3)
        dev_us = float(np.median(dt))
        b_dev = d_best.cpu().numpy()
        # host entry point (upload + kernels + download)
        fm.ComputeDistinctiveDescriptors(offsets=off, desc=desc)
        ht = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            b_host, _m = fm.ComputeDistinctiveDescriptors(offsets=off, desc=desc)
            ht.append((time.perf_counter() - t0) * 1e6)
        host_us = float(np.median(ht))
        # host baseline
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            f.write(np.int64(L).tobytes() + off.tobytes() + desc.tobytes())
        reps = 3 if L * 40 < 2e6 else 1
        base_us = float(subprocess.check_output([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin"), str(reps)]).decode())
        b_base = np.fromfile(os.path.join(tmp, "out.bin"), np.int32)
        n = np.diff(off)
        out["shapes"][name] = {
            "L": L, "observations": int(off[-1]), "N_max": int(n.max()), "pairs": int((n * n).sum()),
            "device_us": round(dev_us, 2), "device_landmarks_per_s": round(L / dev_us * 1e6),
            "host_api_us": round(host_us, 2), "host_api_landmarks_per_s": round(L / host_us * 1e6),
            "host_baseline_us": round(base_us, 2), "host_baseline_landmarks_per_s": round(L / base_us * 1e6),
            "agree": bool(np.array_equal(b_dev, b_host) and np.array_equal(b_dev, b_base)),
        }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
