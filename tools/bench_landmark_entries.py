#!/usr/bin/env python3
"""Batched landmark entry update (hs_landmark_update_entries*, MapPointDBEntry::_updateEntry_, MapPointDB.cpp:223-310): prints one JSON line.

Per shape (L landmarks, N observations each drawn as named, a descriptor set of the same size):
  device_us         hs_landmark_update_entries_device on a caller stream, data resident in HBM, scatter into an hs_landmark array included:
                    device-event time per batch (median of the runs)
  host_api_us       hs_landmark_update_entries from host memory (upload, kernels, download, synchronise): wall time per batch (median)
  host_baseline_us  a single-thread C++ restatement of the reference's four steps (cv::norm as double, float scale-adds and sums, the N x N
                    Hamming matrix with std::sort per row; g++ -O2, compiled by this tool), one landmark after another as hySLAM's mapping thread
                    does after a BA: wall time per batch
and landmarks/s for each.  The three must produce the same sizes, mean distances and descriptors (checked; "agree").
Run on the GPU box: python tools/bench_landmark_entries.py [--runs R]"""
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
from hyslam_amd import _native as N  # noqa: E402

BASELINE_CPP = r"""
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
struct Ent { float pos[3], ref[3]; };
struct Obs { float Ow[3], fx, fy, cx, cy, u, v, sz, ap[3]; int32_t assoc; };
// in.bin: int64 L, Ent[L], int64 ooff[L+1], Obs[..], int64 doff[L+1], desc[..][32] -> out.bin: float mean[L], float size[L], int32 best[L]
static double norm3(const float* v) { double s = 0; for (int k = 0; k < 3; k++) { double x = v[k]; s += x * x; } return std::sqrt(s); }
static int hamming(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int k = 0; k < 32; k += 8) { uint64_t x, y; __builtin_memcpy(&x, a + k, 8); __builtin_memcpy(&y, b + k, 8); d += __builtin_popcountll(x ^ y); }
    return d;
}
template <class T> static void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) exit(2); }
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb"); int64_t L; rd(f, &L, 1);
    std::vector<Ent> ent(L); rd(f, ent.data(), L);
    std::vector<int64_t> ooff(L + 1), doff(L + 1); rd(f, ooff.data(), L + 1);
    std::vector<Obs> obs(ooff[L]); rd(f, obs.data(), obs.size()); rd(f, doff.data(), L + 1);
    std::vector<uint8_t> desc(doff[L] * 32); rd(f, desc.data(), desc.size());
    fclose(f);
    std::vector<float> nrm(3 * L), mind(L), maxd(L), mean(L), size(L); std::vector<int32_t> best(L, -1);
    const int reps = argc > 3 ? atoi(argv[3]) : 1;
    const auto t0 = std::chrono::steady_clock::now();
    for (int rep = 0; rep < reps; rep++)
    for (int64_t l = 0; l < L; l++) {
        const Ent& e = ent[l];
        const Obs* o = obs.data() + ooff[l];
        const int64_t n = ooff[l + 1] - ooff[l];
        if (n > 0) {                                                     // _updateNormalAndDepth_
            float nv[3] = {0, 0, 0};
            for (int64_t j = 0; j < n; j++) {
                float d[3]; for (int k = 0; k < 3; k++) d[k] = e.pos[k] - o[j].Ow[k];
                const float a = (float)(1.0 / norm3(d));
                for (int k = 0; k < 3; k++) { const float t = d[k] * a; nv[k] = t + nv[k]; }
            }
            const float an = (float)(1.0 / (double)n);
            for (int k = 0; k < 3; k++) { const float t = nv[k] * an; nrm[3 * l + k] = t + 0.0f; }
            float pc[3]; for (int k = 0; k < 3; k++) pc[k] = e.pos[k] - e.ref[k];
            const float dist = (float)norm3(pc);
            maxd[l] = 2.0f * dist; mind[l] = 0.5f * dist;
        }
        const int64_t m = doff[l + 1] - doff[l];                       // _computeDistinctiveDescriptor_
        if (m > 0) {
            const uint8_t* d = desc.data() + doff[l] * 32;
            std::vector<float> D(m * m);
            for (int64_t i = 0; i < m; i++) { D[i * m + i] = 0; for (int64_t j = i + 1; j < m; j++) { const float v = (float)hamming(d + i * 32, d + j * 32); D[i * m + j] = v; D[j * m + i] = v; } }
            float bm = std::numeric_limits<float>::max(); int bi = 0;
            for (int64_t i = 0; i < m; i++) {
                std::vector<int> row(D.begin() + i * m, D.begin() + (i + 1) * m);
                std::sort(row.begin(), row.end());
                const int med = row[(size_t)(0.5 * (m - 1))];
                if (med < bm) { bm = med; bi = (int)i; }
            }
            best[l] = bi;
        }
        if (n > 0) {                                                     // _updateMeanDistance_
            float s = 0;
            for (int64_t j = 0; j < n; j++) { float d[3]; for (int k = 0; k < 3; k++) d[k] = e.pos[k] - o[j].Ow[k]; s += (float)norm3(d); }
            mean[l] = s / (float)n;
        }
        float s = 0; int np = 0;                                         // _updateSize_
        for (int64_t j = 0; j < n; j++) {
            float v = -1.0f;
            if (o[j].assoc) {
                float d[3]; for (int k = 0; k < 3; k++) d[k] = o[j].ap[k] - o[j].Ow[k];
                const float z = (float)norm3(d);
                const float r = o[j].sz / 2;
                const float xl = (o[j].u - r - o[j].cx) * (z / o[j].fx), xr = (o[j].u + r - o[j].cx) * (z / o[j].fx);
                const float y = (o[j].v - o[j].cy) * (z / o[j].fy);
                const float len[3] = {xr - xl, y - y, z - z};
                v = (float)norm3(len);
            }
            if (v > 0.0) { s += v; np++; }
        }
        size[l] = s / (float)np;
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
    FILE* w = fopen(argv[2], "wb"); fwrite(mean.data(), 4, L, w); fwrite(size.data(), 4, L, w); fwrite(best.data(), 4, L, w); fclose(w);
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
    T = int(off[-1])
    owner = np.repeat(np.arange(L), n)
    ent = np.zeros(L, N.LM_ENTRY_DTYPE)
    ent["pos"] = rng.normal(0, 10, (L, 3)).astype(np.float32)
    ob = np.zeros(T, N.LM_OBS_DTYPE)
    ob["Ow"] = rng.normal(0, 2, (T, 3)).astype(np.float32)
    ent["ref_Ow"] = ob["Ow"][np.minimum(off[:-1], T - 1)]
    ob["fx"] = ob["fy"] = 700.0
    ob["cx"], ob["cy"] = 640.0, 360.0
    ob["u"], ob["v"] = rng.uniform(0, 1280, T), rng.uniform(0, 720, T)
    ob["kp_size"] = (31.0 * 1.2 ** rng.integers(0, 8, T)).astype(np.float32)
    ob["assoc_pos"] = ent["pos"][owner]
    ob["assoc"] = 1
    # the descriptor set: one per observation, a few centre descriptors with a few flipped bits (views of one point)
    centre = rng.integers(0, 256, (L, 3, 32), dtype=np.uint8)
    desc = centre[owner, rng.integers(0, 3, T)]
    flip = rng.integers(0, 256, (T, 4))
    for k in range(4):
        desc[np.arange(T), flip[:, k] // 8] ^= (1 << (flip[:, k] % 8)).astype(np.uint8)
    return ent, off, ob, np.ascontiguousarray(desc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    args = ap.parse_args()
    shapes = [
        ("L20000_N2-40_plus20_N500-800", dict(seed=1, L=20000, lo=2, hi=40, big=20)),
        ("L20000_N2-40", dict(seed=2, L=20000, lo=2, hi=40)),
        ("L100000_N2-40", dict(seed=3, L=100000, lo=2, hi=40)),
        ("L2000_N2-12", dict(seed=4, L=2000, lo=2, hi=12)),
    ]
    dev = torch.device("cuda", 0)
    ex = HS.ORBExtractor(device=0)
    fm = HS.FeatureMatcher(extractor=ex)
    ts = torch.cuda.Stream()                      # a real stream handle: 0 would mean "the handle's own stream" to the C ABI
    tmp = tempfile.mkdtemp(prefix="bench_lme_")
    exe = os.path.join(tmp, "baseline")
    with open(exe + ".cpp", "w") as f:
        f.write(BASELINE_CPP)
    subprocess.check_call(["g++", "-O2", "-std=c++17", exe + ".cpp", "-o", exe])
    out = {"tool": "bench_landmark_entries", "runs": args.runs, "device": torch.cuda.get_device_name(0),
           "host_baseline": "single-thread C++ restatement of MapPointDB.cpp:223-310 (all four steps), g++ -O2, one landmark at a time",
           "shapes": {}}
    for name, kw in shapes:
        ent, off, ob, desc = make_shape(**kw)
        L = len(ent)
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
        d_in = [to_dev(a) for a in (ent, off, ob, off, desc)]
        d_out = [torch.empty(L * 3, dtype=torch.float32, device=dev)] + [torch.empty(L, dtype=torch.float32, device=dev) for _ in range(4)] + \
                [torch.empty(L, dtype=torch.int32, device=dev) for _ in range(3)]
        d_lms = torch.zeros(L * N.LM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_idx = torch.arange(L, dtype=torch.int32, device=dev)
        run = lambda: ex.landmark_update_entries_device(L, *[t.data_ptr() for t in d_in], *[t.data_ptr() for t in d_out], d_lms=d_lms.data_ptr(),
                                                        d_lm_index=d_idx.data_ptr(), n_lms=L, stream=ts.cuda_stream)
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
        dev_mean, dev_size, dev_best = d_out[3].cpu().numpy(), d_out[4].cpu().numpy(), d_out[5].cpu().numpy()
        # host entry point (upload + kernels + download)
        fm.UpdateLandmarkEntries(ent, obs_offsets=off, obs=ob, desc_offsets=off, desc=desc)
        ht = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            r = fm.UpdateLandmarkEntries(ent, obs_offsets=off, obs=ob, desc_offsets=off, desc=desc)
            ht.append((time.perf_counter() - t0) * 1e6)
        host_us = float(np.median(ht))
        # host baseline
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            f.write(np.int64(L).tobytes() + ent.tobytes() + off.tobytes() + ob.tobytes() + off.tobytes() + desc.tobytes())
        reps = 3 if L * 40 < 2e6 else 1
        base_us = float(subprocess.check_output([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin"), str(reps)]).decode())
        raw = np.fromfile(os.path.join(tmp, "out.bin"), np.uint8)
        b_mean, b_size, b_best = raw[:4 * L].view(np.float32), raw[4 * L:8 * L].view(np.float32), raw[8 * L:].view(np.int32)
        eq = lambda a, b: bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
        n = np.diff(off)
        out["shapes"][name] = {
            "L": L, "observations": int(off[-1]), "N_max": int(n.max()),
            "device_us": round(dev_us, 2), "device_landmarks_per_s": round(L / dev_us * 1e6),
            "host_api_us": round(host_us, 2), "host_api_landmarks_per_s": round(L / host_us * 1e6),
            "host_baseline_us": round(base_us, 2), "host_baseline_landmarks_per_s": round(L / base_us * 1e6),
            "agree": eq(dev_mean, r["mean_dist"]) and eq(dev_mean, b_mean) and eq(dev_size, r["size"]) and eq(dev_size, b_size) and
                     bool(np.array_equal(dev_best, r["best"]) and np.array_equal(dev_best, b_best)),
        }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
