#!/usr/bin/env python3
"""Place-recognition queries (hs_place_query_reloc / _reloc_device, kernels_place.hip) next to a single-thread CPU walk of the reference's own
structures (tools/place_walk_cpu.cpp: inverted file of std::list, std::map merge score; g++ -O2, compiled by this tool).  GPU box.

Databases of 1 000 / 10 000 / 100 000 key frames of ~1 500 words over a 1 000 000-word vocabulary: key frames come in places of 10 that share
1 200 words, 300 words are their own; covisibility = the 10 nearest in sequence; the queries are perturbed copies of stored vectors.  Timed:
  host    hs_place_query_reloc end to end (query + covisibility table copied in, candidates copied out, synchronous), per call
  device  hs_place_query_reloc_device, everything resident, REPS queries back to back on one stream, wall time / REPS after a warm-up and a sync
  cpu     the walk, per query (median of its repeats); not run at 100 000 key frames, where its list and map nodes alone need ~12 GB
Each figure is the median of a run; RUNS runs give the spread.  One JSON line.
usage: bench_place.py [--sizes 1000,10000,100000] [--runs 3] [--reps 20] [--cpu-max 10000]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N_WORDS = 1000000


def make_db(n_kf, seed=1):
    rng = np.random.default_rng(seed)
    n_places = (n_kf + 9) // 10
    base = rng.integers(0, N_WORDS, (n_places, 1200))
    words = np.concatenate([base[np.arange(n_kf) // 10], rng.integers(0, N_WORDS, (n_kf, 300))], 1)
    words.sort(1)
    keep = np.ones(words.shape, bool)
    keep[:, 1:] = words[:, 1:] != words[:, :-1]                              # unique within a key frame
    values = rng.random(words.shape) * 0.2 + 0.9
    off = np.zeros(n_kf + 1, np.int64)
    np.cumsum(keep.sum(1), out=off[1:])
    w, v = words[keep].astype(np.int32), values[keep]
    v /= np.repeat(np.add.reduceat(v, off[:-1]), np.diff(off))
    neigh = np.arange(n_kf)[:, None] + np.array([-5, -4, -3, -2, -1, 1, 2, 3, 4, 5])[None, :]
    neigh = np.where((neigh >= 0) & (neigh < n_kf), neigh, -1).astype(np.int32)
    queries = []
    for j in rng.integers(0, n_kf, 4):
        qw = w[off[j]:off[j + 1]]
        qw = np.unique(np.concatenate([qw[rng.random(len(qw)) < 0.9], rng.integers(0, N_WORDS, 150).astype(np.int32)]))
        qv = rng.random(len(qw)) * 0.2 + 0.9
        queries.append((qw.astype(np.int32), qv / qv.sum()))
    return off, w, v, neigh, queries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,10000,100000")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-max", type=int, default=10000)
    a = ap.parse_args()
    import hipmem
    import hyslam_amd as HS
    from hyslam_amd import _native as N
    ex = HS.ORBExtractor(device=0)
    L = ex._lib
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "place_walk_cpu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "place_walk_cpu.cpp"), "-o", exe])
    out = {"n_words": N_WORDS, "runs": a.runs, "reps": a.reps, "sizes": {}}
    for n_kf in [int(x) for x in a.sizes.split(",")]:
        off, w, v, neigh, queries = make_db(n_kf)
        db = C.c_void_p()
        N.check(ex._h, L.hs_place_db_create(ex._h, N_WORDS, 0, C.byref(db)))
        slot = C.c_int32()
        t0 = time.perf_counter()
        for i in range(n_kf):
            N.check(ex._h, L.hs_place_db_add(db, i + 1, p(w[off[i]:]), p(v[off[i]:]), int(off[i + 1] - off[i]), C.byref(slot)))
        t_add = time.perf_counter() - t0
        cand, n = np.zeros(n_kf, np.int32), C.c_int32()
        d_neigh, d_cand, d_n = hipmem.DevBuf.from_numpy(neigh), hipmem.DevBuf(n_kf * 4), hipmem.DevBuf(4)
        dq = [(hipmem.DevBuf.from_numpy(qw), hipmem.DevBuf.from_numpy(qv), len(qw)) for qw, qv in queries]
        s = hipmem.Stream()
        host_runs, dev_runs, n_cands = [], [], []
        for run in range(a.runs):
            th, td = [], []
            for qi, (qw, qv) in enumerate(queries):
                N.check(ex._h, L.hs_place_query_reloc(db, p(qw), p(qv), len(qw), p(neigh), p(cand), n_kf, C.byref(n), None, None, None, None))   # warm-up
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    N.check(ex._h, L.hs_place_query_reloc(db, p(qw), p(qv), len(qw), p(neigh), p(cand), n_kf, C.byref(n), None, None, None, None))
                    th.append(time.perf_counter() - t0)
                if run == 0:
                    n_cands.append(n.value)
                bw, bv, m = dq[qi]
                for timed in (False, True):
                    s.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.reps):
                        N.check(ex._h, L.hs_place_query_reloc_device(db, bw.ptr, bv.ptr, None, m, d_neigh.ptr, d_cand.ptr, n_kf, d_n.ptr, None, None, None, None, s.ptr))
                    s.synchronize()
                    if timed:
                        td.append((time.perf_counter() - t0) / a.reps)
            host_runs.append(float(np.median(th)) * 1e6)
            dev_runs.append(float(np.median(td)) * 1e6)
        res = {"words_per_kf": float(np.diff(off).mean()), "add_s": round(t_add, 3), "candidates": n_cands,
               "host_us_runs": [round(x, 1) for x in host_runs], "device_us_runs": [round(x, 1) for x in dev_runs]}
        if n_kf <= a.cpu_max:
            path = os.path.join(tmp, "db.bin")
            with open(path, "wb") as f:
                f.write(np.array([N_WORDS, n_kf], np.int32).tobytes() + off.tobytes() + w.tobytes() + v.tobytes() + neigh.tobytes() + np.int32(len(queries)).tobytes())
                for qw, qv in queries:
                    f.write(np.int32(len(qw)).tobytes() + qw.tobytes() + qv.tobytes())
            cpu_runs, cpu_c = [], []
            for run in range(a.runs):
                lines = subprocess.run([exe, path, str(max(3, a.reps // 4))], capture_output=True, text=True, check=True).stdout.strip().split("\n")
                cpu_runs.append(float(np.median([float(l.split(": ")[1].split(" us")[0]) for l in lines])))
                cpu_c = [int(l.split()[-2]) for l in lines]
            os.remove(path)
            res["cpu_walk_us_runs"] = [round(x, 1) for x in cpu_runs]
            res["cpu_walk_candidates"] = cpu_c
        out["sizes"][str(n_kf)] = res
        L.hs_place_db_destroy(db)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
