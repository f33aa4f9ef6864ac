#!/usr/bin/env python3
"""Times one frame of TrackMotionModel + TrackLocalMap on one MI355X, two ways, in the same process and interleaved; reported, not gated:

  resident      hs_track_frame_device: every stage enqueued on one stream over tables resident in HBM; the host reads nothing in between.
  host_driven   the same stages as the library had to be driven before that call existed: the by-value device entry points
                (hs_search_by_projection_device, hs_pose_edges_device, hs_pose_optimize_device, hs_local_map_search_device) with a synchronise, a
                read-back and the host derivation of pose matrices, associations, kp_lm_obs and outlier removal between them, and an upload of what
                the next call reads.  The host decides whether the wide search runs, so it runs only when the narrow one found too few.  The host
                glue here is numpy; `host_glue_ms` is its share (a C++ caller's would be smaller; the synchronise and copy latencies stay).

Shapes: 2 000 key points, a last frame that holds about 1 000 landmarks, a map of 50 000 landmarks and 300 key frames (tools/bench_local_map.py's).
Times are wall clock around a stream synchronise over `--iters` back-to-back frames, median of `--repeats` alternating batches, smallest and largest
beside it.  `without_wide_search_ms` is the same chain enqueued from the public device calls with the narrow search only (measured when the scene's
narrow search suffices, in the same alternation); `wide_search_alone_ms` is the always-enqueued second search by itself.
Both paths must leave the same associations and counts.  Prints one JSON line.
usage: bench_track_frame.py [--iters 200] [--repeats 7] [--keypoints 2000] [--landmarks 50000] [--key-frames 300]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--landmarks", type=int, default=50000)
    ap.add_argument("--key-frames", type=int, default=300)
    a = ap.parse_args()
    import hyslam_amd as HS
    from hyslam_amd import _native as N
    from hyslam_amd.features import _DevBuf
    import ref_track as R
    import track_cases as TC

    n, L, n_kf = a.keypoints, a.landmarks, a.key_frames
    c = TC.build(2024, n=n, n_last=min(n, 1100), extra=L - n, n_kf=n_kf, max_obs=16)
    fr, tp, T = c["frame"], c["tp"], c["T"]
    n_last, cap = len(c["last_kp_lm"]), L
    ex = HS.ORBExtractor(device=0)
    tr = HS.FrameTracker(ex)
    F, fkeep = tr.device_frame(fr)
    KT, tkeep = tr.device_table(T)
    lms = np.ascontiguousarray(c["lms"], N.LM_DTYPE)
    up = lambda x: _DevBuf(ex, np.ascontiguousarray(x).nbytes, np.ascontiguousarray(x))
    d_lms, d_T, d_lk, d_ll, d_ng, d_pa = up(lms), up(c["Tcw_pred"]), up(np.ascontiguousarray(c["last_kps"], N.KP_DTYPE)), up(c["last_kp_lm"]), up(c["neigh"]), up(c["parent"])
    # the state lies in ONE block (kp_lm, kp_lm_obs, n_matches, kp_outl; every piece a multiple of 16 bytes), so that one device copy clears it
    n16 = (n + 15) & ~15

    class View:                                                  # a piece of the block with _DevBuf's read
        def __init__(self, off):
            self.ptr, self.off = block.ptr + off, off

        def read(self, dtype, count):
            return block.read(dtype, count, self.off)
    block = _DevBuf(ex, n16 * 4 * 2 + 16 + n16)
    st = [View(0), View(n16 * 8 + 16), View(n16 * 8), View(n16 * 4)]
    ST = N.TrackState(*[b.ptr for b in st])
    cleared = np.zeros(block.nbytes, np.uint8)
    cleared[:n16 * 8] = 0xFF                                     # kp_lm = kp_lm_obs = -1, n_matches = 0, kp_outl = 0
    d_cleared = up(cleared)
    out, ob = tr.outputs(dict(n=n, n_last=n_last, n_kf=n_kf, cap=cap))
    work = _DevBuf(ex, tr.track_work_bytes(n, n_last, L, cap))
    prm = N.TrackParams(tp.th_motion, tp.th_motion_wide, tp.n_min_matches, tp.th_local, tp.nnratio_motion, tp.nnratio_local, tp.th_high, tp.sigma_ref,
                        tp.n_max_local_keyframes, tp.n_neighbor_keyframes)
    rd = lambda k: ob[k][0].read(ob[k][1], ob[k][2])
    put = lambda buf, x: N.check(ex._h, ex._lib.hs_device_copy(ex._h, buf.ptr, np.ascontiguousarray(x).ctypes.data, np.ascontiguousarray(x).nbytes, 1, None))

    def resident():
        tr.track_frame_device(F, d_T.ptr, d_lk.ptr, d_ll.ptr, n_last, KT, d_lms.ptr, d_ng.ptr, c["neigh"].shape[1], d_pa.ptr, cap, prm, ST, out, work.ptr)

    # ---- the host-driven sequence over the same buffers
    glue = [0.0]
    Fv = N.FrameView.from_buffer_copy(F)
    Fv.kp_lm_obs = st[3].ptr
    cam = np.array([fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["mbf"]], np.float32)
    lm_work = _DevBuf(ex, ex.local_map_work_bytes(L))

    def set_pose(Tcw):                                           # Rcw, tcw, Ow = -Rcw^T tcw on the host
        pv = R.pose_view(Tcw)
        Fv.Rcw[:], Fv.tcw[:], Fv.Ow[:] = pv["Rcw"].tolist(), pv["tcw"].tolist(), pv["Ow"].tolist()
        prob = np.zeros(1, N.POSE_PROBLEM_DTYPE)
        prob["Tcw"][0] = np.asarray(Tcw, np.float32).ravel()
        prob["fx"], prob["fy"], prob["cx"], prob["cy"], prob["bf"] = cam
        return prob

    def optimise(prob, kp_lm, kp_outl, nm, mode, stage):
        put(st[0], kp_lm)
        put(ob["problem"][0], prob)
        ex.pose_edges_device(Fv, d_lms.ptr, L, st[0].ptr, ob["edges_" + stage][0].ptr, n, ob["n_edges_" + stage][0].ptr, tp.sigma_ref)
        ex.pose_optimize_device(1, ob["problem"][0].ptr, ob["edges_" + stage][0].ptr, ob["outlier_" + stage][0].ptr, ob["pose_" + stage][0].ptr, None,
                                ob["n_edges_" + stage][0].ptr, n)
        ex.synchronize()
        res, flags = rd("pose_" + stage)[0], rd("outlier_" + stage)
        t0 = time.perf_counter()
        held = np.nonzero(kp_lm >= 0)[0]                          # the edges are the held views in ascending order
        if res["status"] != N.HS_POSE_TOO_FEW:
            kp_outl[held] = np.where(flags[:len(held)] != 0, 2, 1)
        is_out = np.zeros(n, bool)
        is_out[held] = kp_outl[held] == 2
        count = int((T["lm_nobs"][kp_lm[held]][~is_out[held]] > 0).sum())
        if mode == N.HS_TRACK_MOTION or fr["sensor"] == 1:
            kp_lm[is_out], kp_outl[is_out], nm = -1, 0, nm - int(is_out.sum())
        glue[0] += time.perf_counter() - t0
        return res, count, nm

    def host_driven():
        t0 = time.perf_counter()
        prob = set_pose(c["Tcw_pred"])
        last = R.gather_last(lms, c["last_kp_lm"], c["last_kps"])
        kp_lm, kp_outl, obs = np.full(n, -1, np.int32), np.zeros(n, np.uint8), np.full(n, -1, np.int32)
        glue[0] += time.perf_counter() - t0
        put(ob["last_lms"][0], last)
        put(st[3], obs)
        for th in (tp.th_motion, tp.th_motion_wide):
            pp = N.ProjParams(th, tp.th_high, tp.nnratio_motion, 0.5, 1.5, 0, 1, 1, sigma_ref=tp.sigma_ref)
            N.check(ex._h, ex._lib.hs_search_by_projection_device(ex._h, C.byref(Fv), ob["last_lms"][0].ptr, n_last, C.byref(pp), ob["narrow_idx"][0].ptr,
                                                                  ob["narrow_dist"][0].ptr, ob["narrow_n"][0].ptr, None))
            ex.synchronize()
            nmatches = int(rd("narrow_n")[0])
            if nmatches >= tp.n_min_matches:
                break
        midx = rd("narrow_idx")
        t0 = time.perf_counter()
        kp_lm, kp_outl, nm = R.replay_closed_form(kp_lm, kp_outl, 0, midx, c["last_kp_lm"], L)
        glue[0] += time.perf_counter() - t0
        if nmatches < tp.n_min_matches:
            return None
        res, n_map, nm = optimise(prob, kp_lm, kp_outl, nm, N.HS_TRACK_MOTION, "motion")
        t0 = time.perf_counter()
        prob = set_pose(res["Tcw"].reshape(4, 4))
        bad = (kp_lm >= 0) & (T["lm_bad"][np.maximum(kp_lm, 0)] != 0)
        kp_lm[bad], kp_outl[bad], nm = -1, 0, nm - int(bad.sum())
        obs = np.where(kp_lm >= 0, T["lm_nobs"][np.maximum(kp_lm, 0)], -1).astype(np.int32)
        glue[0] += time.perf_counter() - t0
        put(st[0], kp_lm)
        put(st[3], obs)
        pp = N.ProjParams(tp.th_local, tp.th_high, tp.nnratio_local, 0.5, 1.5, 1, 1, 0, sigma_ref=tp.sigma_ref)
        ex.local_map_search_device(KT, st[0].ptr, n, d_ng.ptr, c["neigh"].shape[1], d_pa.ptr, tp.n_max_local_keyframes, tp.n_neighbor_keyframes, Fv, d_lms.ptr, pp, cap,
                                   out.local, lm_work.ptr)
        ex.synchronize()
        midx, sel = rd("local.match_idx"), rd("local.sel")
        t0 = time.perf_counter()
        kp_lm, kp_outl, nm = R.replay_closed_form(kp_lm, kp_outl, nm, midx, sel, L)
        glue[0] += time.perf_counter() - t0
        res, n_in, nm = optimise(prob, kp_lm, kp_outl, nm, N.HS_TRACK_LOCAL, "local")
        return kp_lm, kp_outl, nm, n_map, n_in

    # ---- both leave the same state
    resident(); ex.synchronize()
    r = rd("result")[0]
    want = (st[0].read(np.int32, n), st[1].read(np.uint8, n), int(st[2].read(np.int32, 1)[0]), int(r["n_matches_map"]), int(r["n_inliers"]))
    used_wide = int(r["used_wide"])
    lm_iters = [int(rd("pose_motion")[0]["lm_iterations"]), int(rd("pose_local")[0]["lm_iterations"])]
    got = host_driven()
    if got is None or any(not np.array_equal(x, y) for x, y in zip(want, got)):
        raise SystemExit("the resident chain and the host-driven sequence disagree")

    # ---- the resident chain WITHOUT the second search, enqueue-only from the public device calls: pose view, clear (one device copy of the
    # cleared block), the narrow search, replay, edges, optimise, discard, then hs_track_local_map_device.  Against hs_track_frame_device it lacks the
    # wide search's launches, the last-frame gather (the records of the call above are reused), the select and the gate.  Valid on a scene whose
    # narrow search suffices: the outputs must equal the resident call's.
    Fn = N.FrameView.from_buffer_copy(F)
    Fn.kp_lm_obs = st[3].ptr
    ppn = N.ProjParams(tp.th_motion, tp.th_high, tp.nnratio_motion, 0.5, 1.5, 0, 1, 1, sigma_ref=tp.sigma_ref)
    off_tcw, off_map = N.POSE_RESULT_DTYPE.fields["Tcw"][1], N.TRACK_RESULT_DTYPE.fields["n_matches_map"][1]

    prob0 = np.zeros(1, N.POSE_PROBLEM_DTYPE)                    # the motion stage's problem, in a buffer nothing else writes
    prob0["Tcw"][0] = np.asarray(c["Tcw_pred"], np.float32).ravel()
    prob0["fx"], prob0["fy"], prob0["cx"], prob0["cy"], prob0["bf"] = cam
    d_prob0 = up(prob0)

    def narrow_only():
        tr.pose_views_device(d_T.ptr, ob["pose_view"][0].ptr)
        ex.debug_stream_copy(block.ptr, d_cleared.ptr, block.nbytes - block.nbytes % 16, 16)
        tr.search_by_projection_posed_device(Fn, ob["pose_view"][0].ptr, ob["last_lms"][0].ptr, n_last, ppn, ob["narrow_idx"][0].ptr, ob["narrow_dist"][0].ptr,
                                             ob["narrow_n"][0].ptr)
        tr.frame_associate_device(n, L, st[0].ptr, st[1].ptr, st[2].ptr, n_last, ob["narrow_idx"][0].ptr, d_ll.ptr, work.ptr)
        ex.pose_edges_device(Fn, d_lms.ptr, L, st[0].ptr, ob["edges_motion"][0].ptr, n, ob["n_edges_motion"][0].ptr, tp.sigma_ref)
        ex.pose_optimize_device(1, d_prob0.ptr, ob["edges_motion"][0].ptr, ob["outlier_motion"][0].ptr, ob["pose_motion"][0].ptr, None,
                                ob["n_edges_motion"][0].ptr, n)
        tr.track_discard_device(N.HS_TRACK_MOTION, ob["edges_motion"][0].ptr, ob["n_edges_motion"][0].ptr, n, ob["outlier_motion"][0].ptr, ob["pose_motion"][0].ptr,
                                KT, fr["sensor"], st[0].ptr, st[1].ptr, st[2].ptr, ob["result"][0].ptr + off_map)
        tr.track_local_map_device(F, ob["pose_motion"][0].ptr + off_tcw, KT, d_lms.ptr, d_ng.ptr, c["neigh"].shape[1], d_pa.ptr, cap, prm, ST, out, work.ptr)

    narrow_ok = not used_wide
    if narrow_ok:
        resident(); ex.synchronize()                             # leaves last_lms as the narrow-only chain reads it
        narrow_only(); ex.synchronize()
        r2 = rd("result")[0]
        got = (st[0].read(np.int32, n), st[1].read(np.uint8, n), int(st[2].read(np.int32, 1)[0]), int(r2["n_matches_map"]), int(r2["n_inliers"]))
        same_work = [int(rd("pose_motion")[0]["lm_iterations"]), int(rd("pose_local")[0]["lm_iterations"])] == lm_iters
        if any(not np.array_equal(x, y) for x, y in zip(want, got)) or not same_work:
            raise SystemExit("the chain without the wide search and the resident chain disagree")

    def batch(call):
        t0 = time.perf_counter()
        for _ in range(a.iters):
            call()
        ex.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.iters

    t_res, t_host, t_glue, t_narrow = [], [], [], []
    for _ in range(a.repeats):                                    # interleaved: the machine's other work hits both alike
        t_res.append(batch(resident))
        glue[0] = 0.0
        t_host.append(batch(host_driven))
        t_glue.append(glue[0] * 1e3 / a.iters)
        if narrow_ok:
            t_narrow.append(batch(narrow_only))
    if narrow_ok and [int(rd("pose_motion")[0]["lm_iterations"]), int(rd("pose_local")[0]["lm_iterations"])] != lm_iters:
        raise SystemExit("the timed chain without the wide search did other work than the resident chain")
    ppw = N.ProjParams(tp.th_motion_wide, tp.th_high, tp.nnratio_motion, 0.5, 1.5, 0, 1, 1, sigma_ref=tp.sigma_ref)
    Fs = N.FrameView.from_buffer_copy(F)
    Fs.kp_lm_obs = st[3].ptr
    wide = lambda: tr.search_by_projection_posed_device(Fs, ob["pose_view"][0].ptr, ob["last_lms"][0].ptr, n_last, ppw, ob["wide_idx"][0].ptr, ob["wide_dist"][0].ptr,
                                                        ob["wide_n"][0].ptr)
    wide(); ex.synchronize()
    t_wide = [batch(wide) for _ in range(a.repeats)]
    med = lambda v: round(float(np.median(v)), 4)
    span = lambda v: [round(float(min(v)), 4), round(float(max(v)), 4)]
    res = dict(keypoints=n, last_frame_keypoints=n_last, last_frame_landmarks=int((c["last_kp_lm"] >= 0).sum()), landmarks=L, key_frames=n_kf, cap=cap, iters=a.iters,
               repeats=a.repeats, used_wide=used_wide, n_narrow=int(r["n_narrow"]), n_wide=int(r["n_wide"]), n_matches_map=want[3], n_inliers=want[4],
               n_edges=[int(rd("n_edges_motion")[0]), int(rd("n_edges_local")[0])], lm_iterations=lm_iters,
               resident_ms=med(t_res), resident_min_max_ms=span(t_res), host_driven_ms=med(t_host), host_driven_min_max_ms=span(t_host), host_glue_ms=med(t_glue),
               wide_search_alone_ms=med(t_wide), without_wide_search_ms=med(t_narrow) if narrow_ok else None,
               without_wide_search_min_max_ms=span(t_narrow) if narrow_ok else None)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
