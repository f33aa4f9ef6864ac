#!/usr/bin/env python3
"""Times TrackLocalMap's UpdateLocalMap + SearchLocalPoints on one MI355X in BASELINE config 4's shape — a 1920 x 1080 stereo frame of about 2 000
key points, a map of 50 000 landmarks and 300 key frames — two ways, reported, not gated:

  device_chain   hs_local_map_search_device: vote, key-frame expansion, landmark selection, gather and projection search on one stream over tables
                 resident in HBM (the observation table, the hs_landmark records, the frame the extractor left on the device).  Median over
                 `--repeats` batches of `--iters` back-to-back calls, wall clock around a stream synchronise, so launch overhead is inside; the
                 stages alone are timed the same way.  The smallest and largest batch are printed beside the median.
  host_path      the path before this call existed, for the same work: (1) the host assembly of the local map, i.e. the std::set walks of
                 UpdateLocalKeyFrames / UpdateLocalPoints and the filter of SearchLocalPoints over the map's objects — the literal restatement of
                 tests/cpp/localmap_restatement.h on objects built from the SAME table (tests/cpp/bench_localmap_ref.cpp, g++ -O2, one core, median);
                 (2) SearchByProjection through the adaptor on 50 000 landmarks: tests/cpp/bench_adaptor's `TrackLocalMap_SearchByProjection_ms`
                 (gather of the MapPoint fields, C ABI call, association replay).  Both on cv_compat.h's stand-ins for hySLAM's classes.

The frame holds landmarks from all over the map, so nearly every key frame is local and the selection is about as long as the table: the device chain
then searches as many real landmarks as bench_adaptor does.  The counts of the restatement must equal the device's.  Prints one JSON line.
usage: bench_local_map.py [--iters 2000] [--repeats 7] [--landmarks 50000] [--key-frames 300]"""
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
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--landmarks", type=int, default=50000)
    ap.add_argument("--key-frames", type=int, default=300)
    ap.add_argument("--host-path", type=int, choices=[0, 1], default=1, help="0: skip the two CPU-side programs")
    a = ap.parse_args()
    import torch
    import hyslam_amd as HS
    from hyslam_amd import _native as N
    from hyslam_amd.synth import synth_local_map, synth_stereo_pair
    from kfgraph_cases import key_frame_queries, random_table
    import ref_localmap as R
    dev = torch.device("cuda", 0)
    W, H, L, n_kf, fx = 1920, 1080, a.landmarks, a.key_frames, 1050.0
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    mk = lambda n, dt=torch.uint8: torch.zeros(max(n, 1), dtype=dt, device=dev)

    # ---- the frame: extracted and stereo-matched on the device, left there
    ex = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=2000), device=0)
    m = HS.FeatureMatcher(extractor=ex)
    Limg, Rimg = synth_stereo_pair(1000, W, H)
    left, right = torch.from_numpy(Limg).to(dev), torch.from_numpy(Rimg).to(dev)
    ex.reserve(W, H, 2)
    cap_kp, kb = ex.max_keypoints(), N.KP_DTYPE.itemsize
    kL, kR, dL, dR, nL, nR = mk(cap_kp * kb), mk(cap_kp * kb), mk(cap_kp * 32), mk(cap_kp * 32), mk(1, torch.int32), mk(1, torch.int32)
    uR, depth = mk(cap_kp, torch.float32), mk(cap_kp, torch.float32)
    sp = HS.stereo_params(HS.Camera(fx=fx, mbf=fx * 0.12, mnMaxY=float(H)))
    s = torch.cuda.Stream()
    ex.stereo_frontend_batch_device(left.data_ptr(), right.data_ptr(), 1, W, H, W, W * H, kL.data_ptr(), dL.data_ptr(), nL.data_ptr(), kR.data_ptr(),
                                    dR.data_ptr(), nR.data_ptr(), cap_kp, sp, uR.data_ptr(), depth.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    n0 = int(nL.item())
    kps0 = kL.cpu().numpy().view(N.KP_DTYPE)[:n0]
    lms = synth_local_map(kps0, dL.cpu().numpy().reshape(-1, 32)[:n0], depth.cpu().numpy()[:n0], L, 77, fx, fx, W / 2 - 0.5, H / 2 - 0.5)
    obs = torch.full((cap_kp,), -1, dtype=torch.int32, device=dev)
    F = N.FrameView()
    for i, v in enumerate(np.eye(3, dtype=np.float32).reshape(-1)):
        F.Rcw[i] = float(v)
    F.fx, F.fy, F.cx, F.cy, F.mbf, F.sensor = fx, fx, W / 2 - 0.5, H / 2 - 0.5, fx * 0.12, 1
    F.min_x, F.max_x, F.min_y, F.max_y, F.size_ref, F.n = 0.0, float(W), 0.0, float(H), 31.0, n0
    F.kps, F.desc, F.uR, F.kp_lm_obs = kL.data_ptr(), dL.data_ptr(), uR.data_ptr(), obs.data_ptr()
    pp = N.ProjParams(5.0, 100.0, 0.8, 0.5, 1.5, 1, 1, 0)

    # ---- the map: every landmark seen by a run of up to 16 consecutive key frames; each key frame hangs on its predecessor; the neighbour lists are
    # the ordered rows of a whole-graph recompute; the frame holds a landmark on 70 % of its key points
    T = random_table(1, n_kf, L, max_obs=16, window=True, p_bad_lm=0.02)
    off, q_lm, ids = key_frame_queries(T)
    neigh = np.ascontiguousarray(m.KeyFrameVotes(T, q_offsets=off, q_lm=q_lm, self_id=ids, th=15, cap=10, weights=False)["ordered_slot"], np.int32)
    parent = np.arange(-1, n_kf - 1, dtype=np.int32)
    rng = np.random.default_rng(5)
    flm = np.full(n0, -1, np.int32)
    held = rng.random(n0) < 0.7
    flm[held] = rng.choice(L, int(held.sum()), replace=False)
    order = ("lm_obs_offsets", "lm_obs_kf", "lm_obs_octave", "lm_bad", "lm_nobs", "kf_bad", "kf_id")
    keep = [up(T[k]) for k in order]
    KT = N.KfTable(L, n_kf, *[b.data_ptr() for b in keep])
    d_flm, d_neigh, d_parent, d_lms = up(flm), up(neigh), up(parent), up(lms)
    cap = L
    o = dict(weights=mk(n_kf * 4), max_slot=mk(4), max_count=mk(4), local=mk(n_kf), n_local=mk(4), frame_remove=mk(n0), sel=mk(cap * 4), n_sel=mk(4),
             lms=mk(cap * 80), match_idx=mk(cap * 4), match_dist=mk(cap * 4), n_matches=mk(4))
    out = N.LocalMapOut(*[o[k].data_ptr() for k, _ in N.LocalMapOut._fields_])
    work = mk(ex.local_map_work_bytes(L))
    q_off, n_ord = up(np.array([0, n0], np.int64)), mk(4)
    sp_ = s.cuda_stream

    def timed(call):
        call(); s.synchronize()
        ms = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(a.iters):
                call()
            s.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / a.iters)
        return round(float(np.median(ms)), 4), [round(float(min(ms)), 4), round(float(max(ms)), 4)]

    chain = lambda: ex.local_map_search_device(KT, d_flm.data_ptr(), n0, d_neigh.data_ptr(), 10, d_parent.data_ptr(), 80, 10, F, d_lms.data_ptr(), pp, cap,
                                               out, work.data_ptr(), sp_)
    res = dict(frame="%dx%d" % (W, H), keypoints=n0, landmarks=L, key_frames=n_kf, observations=int(T["lm_obs_offsets"][-1]), associations=int(held.sum()),
               cap=cap, iters=a.iters, repeats=a.repeats)
    res["device_chain_ms"], res["device_chain_min_max_ms"] = timed(chain)
    stages = dict(
        vote=lambda: N.check(ex._h, ex._lib.hs_kf_votes_device(ex._h, C.byref(KT), 1, q_off.data_ptr(), d_flm.data_ptr(), None, 1, 1, out.weights, out.max_slot,
                                                               out.max_count, None, None, 0, n_ord.data_ptr(), sp_)),
        local_keyframes=lambda: ex.local_keyframes_device(n_kf, out.weights, KT.kf_bad, d_neigh.data_ptr(), 10, d_parent.data_ptr(), 80, 10, out.local, out.n_local, sp_),
        local_points=lambda: ex.local_points_device(KT, out.local, d_flm.data_ptr(), n0, out.frame_remove, out.sel, cap, out.n_sel, work.data_ptr(), sp_),
        gather=lambda: ex.landmark_gather_device(d_lms.data_ptr(), L, out.sel, out.n_sel, cap, out.lms, sp_),
        projection_search=lambda: N.check(ex._h, ex._lib.hs_search_by_projection_device(ex._h, C.byref(F), out.lms, cap, C.byref(pp), out.match_idx, out.match_dist,
                                                                                        out.n_matches, sp_)))
    res["device_stage_ms"] = {k: timed(f)[0] for k, f in stages.items()}
    # the search alone on the ungathered table: what the parent commit's device path runs once the host has assembled the records
    res["projection_search_on_table_ms"] = timed(lambda: N.check(ex._h, ex._lib.hs_search_by_projection_device(
        ex._h, C.byref(F), d_lms.data_ptr(), L, C.byref(pp), out.match_idx, out.match_dist, out.n_matches, sp_)))[0]
    chain(); s.synchronize()
    rd = lambda k, dt: o[k].cpu().numpy().view(dt)
    sel, n_sel = rd("sel", np.int32)[:cap], int(rd("n_sel", np.int32)[0])
    got = dict(n_local=int(rd("n_local", np.int32)[0]), n_sel=n_sel, sum_sel=int(sel[:n_sel].astype(np.int64).sum()), n_removed=int(rd("frame_remove", np.uint8)[:n0].sum()))
    res.update(got, matches=int(rd("n_matches", np.int32)[0]))
    # the device's selection against the numpy restatement (tests/ref_localmap.py)
    local_ref, _ = R.local_keyframes_fast(rd("weights", np.int32)[:n_kf], T["kf_bad"], neigh, parent, 80, 10)
    want = R.local_points_fast(T, local_ref, flm, cap)
    if want["n_sel"] != n_sel or not np.array_equal(want["sel"], sel) or not np.array_equal(local_ref, rd("local", np.uint8)[:n_kf]):
        raise SystemExit("the device chain and tests/ref_localmap.py disagree")

    if a.host_path:
        cpp = os.path.join(ROOT, "tests", "cpp")
        with tempfile.TemporaryDirectory() as tmp:
            exe, data = os.path.join(tmp, "bench_localmap_ref"), os.path.join(tmp, "table.bin")
            subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(cpp, "bench_localmap_ref.cpp"), "-o", exe])
            with open(data, "wb") as f:
                np.array([L, n_kf, len(T["lm_obs_kf"]), n0, 10, 9, 80, 10], np.int64).tofile(f)
                for x, t in ((T["lm_obs_offsets"], np.int64), (T["lm_obs_kf"], np.int32), (T["lm_bad"], np.uint8), (T["kf_bad"], np.uint8), (neigh, np.int32),
                             (parent, np.int32), (flm, np.int32)):
                    np.ascontiguousarray(x, t).tofile(f)
            cpu = json.loads(subprocess.check_output([exe, data]))
            if any(cpu[k] != v for k, v in got.items()):
                raise SystemExit("the literal restatement and the device disagree: %r vs %r" % (cpu, got))
            bexe, fl, fr = os.path.join(tmp, "bench_adaptor"), os.path.join(tmp, "L.raw"), os.path.join(tmp, "R.raw")
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(cpp, "bench_adaptor.cpp"), "-o", bexe,
                                   "-L" + os.path.join(ROOT, "hyslam_amd"), "-lhyslam_amd", "-Wl,-rpath," + os.path.join(ROOT, "hyslam_amd")])
            Limg.tofile(fl); Rimg.tofile(fr)
            t = json.loads(subprocess.check_output([bexe, str(W), str(H), fl, fr, "20", str(L)], timeout=600))["TrackLocalMap_SearchByProjection_ms"]
        res["host_path"] = dict(assembly_ms=cpu["assembly_ms"], search_through_adaptor_ms=t["total"],
                                search_split_ms=dict(gather=t["gather"], c_abi=t["c_abi"], scatter=t["scatter"], landmarks=t["landmarks"], matches=t["matches"]),
                                total_ms=round(cpu["assembly_ms"] + t["total"], 4), host_gather_ms=t["gather"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
