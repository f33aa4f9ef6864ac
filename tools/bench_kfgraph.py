#!/usr/bin/env python3
"""Times the key-frame graph entry points (hs_kf_votes_device, hs_kf_redundancy_device) on one MI355X — reported, not gated:

  whole_graph   UpdateConnections for every key frame of a map: 500 key frames, 100 000 landmarks seen by runs of consecutive key frames
  local_votes   one UpdateLocalKeyFrames-shaped query (2 000 matched landmarks, bad key frames counted)
  culler        one KeyFrameCuller-shaped call: 50 candidates with the landmarks they observe
  ranked_list   one query whose ordered list is longer than HS_KF_SORT_PASS (every one of HS_KF_LDS_SLOTS, and of one more, key frames listed)

Device forms on one stream, inputs resident; every figure is the median over `--repeats` batches of `--iters` back-to-back calls (wall clock around
a stream synchronise, so launch overhead is inside).  The host forms (upload + kernel + download + synchronise) are timed once per call as well.
Beside them, under "cpu_std_map", the std::map restatement of the reference's three functions (tests/cpp/kfgraph_restatement.h, the one the adaptor
test compares with) walks objects built from the same table: tests/cpp/bench_kfgraph_ref.cpp, compiled here with g++ -O2 and run on one CPU core;
its sums must equal those of the device's results.  Prints one JSON line.  usage: bench_kfgraph.py [--iters 50] [--repeats 7]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--key-frames", type=int, default=500)
    ap.add_argument("--landmarks", type=int, default=100000)
    a = ap.parse_args()
    import hipmem
    import hyslam_amd as HS
    from hyslam_amd import _native as N
    from kfgraph_cases import key_frame_queries, random_candidates, random_table, table
    m = HS.FeatureMatcher(extractor=HS.ORBExtractor(device=0))
    ex = m._ex
    T = random_table(1, a.key_frames, a.landmarks, max_obs=16, window=True)
    off, q_lm, ids = key_frame_queries(T)
    n_kf, Q = a.key_frames, a.key_frames
    order = ("lm_obs_offsets", "lm_obs_kf", "lm_obs_octave", "lm_bad", "lm_nobs", "kf_bad", "kf_id")
    keep = [hipmem.DevBuf.from_numpy(T[k]) for k in order]
    KT = N.KfTable(a.landmarks, n_kf, *[b.ptr for b in keep])
    s = hipmem.Stream()

    def timed(call):
        call(); s.synchronize()
        ms = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(a.iters):
                call()
            s.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / a.iters)
        return float(np.median(ms)), float(min(ms))

    res = dict(key_frames=n_kf, landmarks=a.landmarks, observations=int(T["lm_obs_offsets"][-1]), iters=a.iters, repeats=a.repeats)
    # whole-graph recompute
    ins = [hipmem.DevBuf.from_numpy(x) for x in (off, q_lm, ids)]
    outs = [hipmem.DevBuf(Q * n_kf * 4)] + [hipmem.DevBuf(Q * 4) for _ in range(2)] + [hipmem.DevBuf(Q * 10 * 4) for _ in range(2)] + [hipmem.DevBuf(Q * 4)]
    votes = lambda Qn, i, o, bad, w: N.check(ex._h, ex._lib.hs_kf_votes_device(ex._h, C.byref(KT), Qn, i[0].ptr, i[1].ptr, i[2].ptr, bad, 15, w, o[1].ptr, o[2].ptr,
                                                                              o[3].ptr, o[4].ptr, 10, o[5].ptr, s.ptr))
    res["whole_graph_ms"], res["whole_graph_min_ms"] = timed(lambda: votes(Q, ins, outs, 0, outs[0].ptr))
    res["whole_graph_no_weights_ms"], _ = timed(lambda: votes(Q, ins, outs, 0, None))
    res["whole_graph_query_landmarks"] = int(len(q_lm))
    # one local-map vote
    rng = np.random.default_rng(2)
    lq = rng.choice(a.landmarks, 2000, replace=False).astype(np.int32)
    lin = [hipmem.DevBuf.from_numpy(x) for x in (np.array([0, 2000], np.int64), lq, np.array([-1], np.int64))]
    res["local_votes_ms"], res["local_votes_min_ms"] = timed(lambda: votes(1, lin, outs, 1, outs[0].ptr))
    # culler: 50 candidates = 50 key frames with the landmarks they observe
    cand_kf = rng.choice(n_kf, 50, replace=False)
    sizes = [int(off[k + 1] - off[k]) for k in cand_kf]
    cand = random_candidates(3, T, sizes)
    cand["cand_slot"] = cand_kf.astype(np.int32)
    cand["item_lm"] = np.concatenate([q_lm[off[k]:off[k + 1]] for k in cand_kf]).astype(np.int32)
    owner = np.repeat(np.arange(a.landmarks), np.diff(T["lm_obs_offsets"]))
    kp_octave = T["lm_obs_octave"][np.lexsort((owner, T["lm_obs_kf"]))]                  # a key frame's key points, in the order of its query
    cand["item_octave"] = np.concatenate([kp_octave[off[k]:off[k + 1]] for k in cand_kf]).astype(np.int32)
    cin = [hipmem.DevBuf.from_numpy(cand[k]) for k in ("cand_slot", "cand_th_depth", "cand_offsets", "item_lm", "item_octave", "item_depth")]
    couts = [hipmem.DevBuf(256) for _ in range(3)]
    res["culler_ms"], res["culler_min_ms"] = timed(lambda: N.check(ex._h, ex._lib.hs_kf_redundancy_device(
        ex._h, C.byref(KT), 50, *[b.ptr for b in cin], 0, 3, 0.9, *[o.ptr for o in couts], s.ptr)))
    res["culler_items"] = int(sum(sizes))
    # the rank fallback of the ordered list: every key frame listed (one landmark each, th = 1), more than HS_KF_SORT_PASS of them, with the
    # counters in LDS (n_kf = HS_KF_LDS_SLOTS) and in global memory (one more)
    for name, n in (("ranked_list_lds_ms", N.HS_KF_LDS_SLOTS), ("ranked_list_global_ms", N.HS_KF_LDS_SLOTS + 1)):
        R = table(n, [[i] for i in range(n)])
        rk = [hipmem.DevBuf.from_numpy(R[k]) for k in order]
        RT = N.KfTable(n, n, *[b.ptr for b in rk])
        rin = [hipmem.DevBuf.from_numpy(x) for x in (np.array([0, n], np.int64), np.arange(n, dtype=np.int32))]
        rw = hipmem.DevBuf(n * 4)
        call = lambda: N.check(ex._h, ex._lib.hs_kf_votes_device(ex._h, C.byref(RT), 1, rin[0].ptr, rin[1].ptr, None, 0, 1, rw.ptr, outs[1].ptr, outs[2].ptr,
                                                                 outs[3].ptr, outs[4].ptr, 10, outs[5].ptr, s.ptr))
        call(); s.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            call()
        s.synchronize()
        res[name] = (time.perf_counter() - t0) * 1e3 / 3
    # host forms: one call each, staging included
    def host(f, n=5):
        f()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter(); f(); ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))
    got = {}
    res["host_whole_graph_ms"] = host(lambda: got.update(w=m.KeyFrameVotes(T, q_offsets=off, q_lm=q_lm, self_id=ids)))
    res["host_local_votes_ms"] = host(lambda: got.update(l=m.KeyFrameVotes(T, queries=[lq], count_bad_kf=True)))
    res["host_culler_ms"] = host(lambda: got.update(c=m.KeyFrameRedundancy(T, cand["cand_slot"], cand["cand_th_depth"], cand_offsets=cand["cand_offsets"],
                                                                           item_lm=cand["item_lm"], item_octave=cand["item_octave"], item_depth=cand["item_depth"])))
    # the std::map restatement on the same table
    cpp = os.path.join(ROOT, "tests", "cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe, data = os.path.join(tmp, "bench_kfgraph_ref"), os.path.join(tmp, "table.bin")
        subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(cpp, "bench_kfgraph_ref.cpp"), "-o", exe])
        with open(data, "wb") as f:
            np.array([a.landmarks, n_kf, len(T["lm_obs_kf"]), len(lq), 50, len(cand["item_lm"]), 15, 3, 3], np.int64).tofile(f)
            for x, t in ((T["lm_obs_offsets"], np.int64), (T["lm_obs_kf"], np.int32), (T["lm_obs_octave"], np.int32), (T["lm_bad"], np.uint8),
                         (T["lm_nobs"], np.int32), (T["kf_bad"], np.uint8), (T["kf_id"], np.int64), (lq, np.int32), (cand["cand_slot"], np.int32),
                         (cand["cand_th_depth"], np.float32), (cand["cand_offsets"], np.int64), (cand["item_depth"], np.float32)):
                np.ascontiguousarray(x, t).tofile(f)
        cpu = json.loads(subprocess.check_output([exe, data]))
    w, l, c = got["w"], got["l"], got["c"]
    dev = dict(sum_weights=int(w["weights"].sum()), sum_max_count=int(w["max_count"].sum()), sum_n_ordered=int(w["n_ordered"].sum()),
               local_sum_weights=int(l["weights"].sum()), local_max_count=int(l["max_count"][0]), sum_n_mps=int(c["n_mps"].sum()),
               sum_n_redundant=int(c["n_redundant"].sum()), n_cull=int(c["cull"].sum()))
    if any(cpu[k] != v for k, v in dev.items()):
        raise SystemExit("the std::map restatement and the device disagree: %r vs %r" % (cpu, dev))
    res["cpu_std_map"] = cpu
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
