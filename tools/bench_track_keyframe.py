#!/usr/bin/env python3
"""Times what follows the two track functions for one frame — reference key-frame vote, key-frame decision, stereo landmark creation, outlier
removal — on one MI355X, two ways, in the same process and interleaved; reported, not gated:

  resident      hs_track_keyframe_device enqueued on the state, the pose and the 32-byte result hs_track_frame_device left in HBM; the host reads
                the 64-byte hs_keyframe_result at the end.
  host_driven   the same work as a caller had to do it before that call existed: synchronise, download kp_lm, kp_outl, n_matches, the depths, the
                track result and the pose, run the numpy restatement (tests/ref_keyframe.py, dense), upload kp_lm, kp_outl, n_matches and
                kp_lm_obs.  `host_glue_ms` is the restatement's share (a C++ caller's would be smaller; the synchronise and copy latencies stay).
                The creation records are not uploaded: the host keeps them.

hs_track_frame_device runs once; every timed iteration first restores the state it left with one device copy (`restore_copy_ms`, timed alone and
NOT subtracted from the other figures), so both ways start from the same bytes every time.  Two configurations: an inserting frame (the key-frame
interval is exceeded) and a non-inserting one (nothing asks for a key frame: stage 5's kernels return at their gate).  `stage_ms` times each stage's
entry point after the same restore copy, the copy's own time subtracted; `launches` is the kernel count per stage.
Shapes: 2 000 key points, 50 000 landmarks, 300 key frames (tools/bench_track_frame.py's).  Wall clock around a stream synchronise over `--iters`
back-to-back iterations, median of `--repeats` alternating batches, smallest and largest beside it.  Both ways must leave the same state.  One JSON line.
usage: bench_track_keyframe.py [--iters 200] [--repeats 7] [--keypoints 2000] [--landmarks 50000] [--key-frames 300]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LAUNCHES = {1: 4, 2: 1, 3: 1, 4: 1, 5: 3, 6: 1}


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
    import keyframe_cases as KC
    import ref_keyframe as RKF
    import track_cases as TC

    n, L, n_kf = a.keypoints, a.landmarks, a.key_frames
    c = TC.build(2024, n=n, n_last=min(n, 1100), extra=L - n, n_kf=n_kf, max_obs=16)
    fr, tp, T = c["frame"], c["tp"], c["T"]
    n_last, cap = len(c["last_kp_lm"]), L
    ex = HS.ORBExtractor(device=0)
    tr = HS.FrameTracker(ex)
    F, fkeep = tr.device_frame(fr)
    KT, tkeep = tr.device_table(T)
    up = lambda x: _DevBuf(ex, np.ascontiguousarray(x).nbytes, np.ascontiguousarray(x))
    d_lms, d_T, d_lk, d_ll = up(np.ascontiguousarray(c["lms"], N.LM_DTYPE)), up(c["Tcw_pred"]), up(np.ascontiguousarray(c["last_kps"], N.KP_DTYPE)), up(c["last_kp_lm"])
    d_ng, d_pa = up(c["neigh"]), up(c["parent"])
    # the state in ONE block (kp_lm, kp_lm_obs, n_matches, kp_outl; every piece a multiple of 16 bytes): one device copy restores it
    n16 = (n + 15) & ~15
    block, saved = _DevBuf(ex, n16 * 9 + 16), _DevBuf(ex, n16 * 9 + 16)
    off = dict(kp_lm=0, kp_lm_obs=n16 * 4, n_matches=n16 * 8, kp_outl=n16 * 8 + 16)
    ST = N.TrackState(block.ptr + off["kp_lm"], block.ptr + off["kp_outl"], block.ptr + off["n_matches"], block.ptr + off["kp_lm_obs"])
    tout, tob = tr.outputs(dict(n=n, n_last=n_last, n_kf=n_kf, cap=cap))
    twork = _DevBuf(ex, tr.track_work_bytes(n, n_last, L, cap))
    tprm = N.TrackParams(tp.th_motion, tp.th_motion_wide, tp.n_min_matches, tp.th_local, tp.nnratio_motion, tp.nnratio_local, tp.th_high, tp.sigma_ref,
                         tp.n_max_local_keyframes, tp.n_neighbor_keyframes)
    tr.track_frame_device(F, d_T.ptr, d_lk.ptr, d_ll.ptr, n_last, KT, d_lms.ptr, d_ng.ptr, c["neigh"].shape[1], d_pa.ptr, cap, tprm, ST, tout, twork.ptr)
    ex.synchronize()
    nbytes = block.nbytes - block.nbytes % 16
    ex.debug_stream_copy(saved.ptr, block.ptr, nbytes, 16)
    ex.synchronize()
    d_track, d_pose = tob["result"][0], tob["pose_local"][0]
    d_Tcw = d_pose.ptr + N.POSE_RESULT_DTYPE.fields["Tcw"][1]

    # the frame's depths (the stereo matcher's output in an integration) and the key frames' associations
    with np.errstate(all="ignore"):
        depth = np.where(fr["uR"] > 0, np.float32(fr["mbf"]) / (fr["kps"]["x"] - fr["uR"]).astype(np.float32), np.float32(-1)).astype(np.float32)
    rng = np.random.default_rng(9)
    K = KC.keyframes([rng.integers(-1, L, n).tolist() for _ in range(n_kf)])
    KF, kkeep = tr.device_keyframes(dict(K, kps=np.zeros(n * n_kf, N.KP_DTYPE), desc=np.zeros((n * n_kf, 32), np.uint8), node=np.full(n * n_kf, -1, np.int32)))
    d_depth, d_ref = up(depth), up(np.array([0], np.int32))
    new_cap = n
    out, ob = tr.keyframe_outputs(new_cap)
    work = _DevBuf(ex, tr.keyframe_work_bytes(n, n_kf, new_cap))
    th_depth = float(np.median(depth[depth > 0]))
    configs = dict(inserting=RKF.params(frame_id=100, last_keyframe_id=10, th_depth=th_depth, thresh_init=5, thresh_refine=5),
                   not_inserting=RKF.params(frame_id=12, last_keyframe_id=10, th_depth=th_depth, thresh_init=5, thresh_refine=5, N_tracked_target=0,
                                            min_N_tracked_close=0))
    restore = lambda: ex.debug_stream_copy(block.ptr, saved.ptr, nbytes, 16)
    rd_state = lambda: (block.read(np.int32, n, off["kp_lm"]), block.read(np.uint8, n, off["kp_outl"]), int(block.read(np.int32, 1, off["n_matches"])[0]),
                        block.read(np.int32, n, off["kp_lm_obs"]))
    put = lambda ptr, x: N.check(ex._h, ex._lib.hs_device_copy(ex._h, ptr, np.ascontiguousarray(x).ctypes.data, np.ascontiguousarray(x).nbytes, 1, None))

    def batch(call):
        t0 = time.perf_counter()
        for _ in range(a.iters):
            call()
        ex.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.iters

    med = lambda v: round(float(np.median(v)), 4)
    span = lambda v: [round(float(min(v)), 4), round(float(max(v)), 4)]
    res = dict(keypoints=n, landmarks=L, key_frames=n_kf, views_with_depth=int((depth > 0).sum()), iters=a.iters, repeats=a.repeats, launches=LAUNCHES)
    for name, p in configs.items():
        prm = N.KeyFrameParams(**p)
        glue = [0.0]

        def resident():
            restore()
            tr.track_keyframe_device(F, d_depth.ptr, d_Tcw, KT, KF, d_track.ptr, prm, ST, d_ref.ptr, new_cap, out, work.ptr)

        def host_driven():
            restore()
            ex.synchronize()
            kp_lm, kp_outl, nm, _ = rd_state()
            z = d_depth.read(np.float32, n)
            t, pose = d_track.read(N.TRACK_RESULT_DTYPE, 1)[0], d_pose.read(N.POSE_RESULT_DTYPE, 1)[0]
            t0 = time.perf_counter()
            case = dict(state=(kp_lm, kp_outl, nm), T=T, K=K, depth=z, frame=fr, Tcw=pose["Tcw"].reshape(4, 4), prm=p, ref_slot=0, new_cap=new_cap,
                        track=dict(status=int(t["status"]), n_matches_map=int(t["n_matches_map"]), n_inliers=int(t["n_inliers"])))
            r = RKF.dense(case)
            glue[0] += time.perf_counter() - t0
            put(block.ptr + off["kp_lm"], r["kp_lm"])
            put(block.ptr + off["kp_outl"], r["kp_outl"])
            put(block.ptr + off["n_matches"], np.array([r["n_matches"]], np.int32))
            put(block.ptr + off["kp_lm_obs"], r["kp_lm_obs"])
            return r

        def stage(s):
            if s == 1:
                tr.keyframe_reference_device(n, ST, KT, d_ref.ptr, ob["result"][0].ptr, work.ptr)
            elif s == 2:
                tr.keyframe_gate_device(d_track.ptr, prm, ob["result"][0].ptr)
            elif s == 3:
                tr.keyframe_clean_device(n, ST, KT, ob["result"][0].ptr)
            elif s == 4:
                tr.keyframe_need_device(n, F.sensor, d_depth.ptr, ST, KT, KF, d_ref.ptr, d_track.ptr, prm, ob["result"][0].ptr)
            elif s == 5:
                tr.keyframe_create_device(F, d_depth.ptr, d_Tcw, ST, KT, prm, new_cap, out, work.ptr)
            else:
                tr.keyframe_discard_device(n, ST, ob["result"][0].ptr)

        put(d_ref.ptr, np.array([0], np.int32))
        resident(); ex.synchronize()
        want, kr = rd_state(), ob["result"][0].read(N.KEYFRAME_RESULT_DTYPE, 1)[0]
        put(d_ref.ptr, np.array([0], np.int32))
        r = host_driven()
        got = rd_state()
        if any(not np.array_equal(x, y) for x, y in zip(want, got)) or {k: int(kr[k]) for k in RKF.RESULT_KEYS} != r["result"]:
            raise SystemExit("the resident call and the host-driven sequence disagree (%s)" % name)
        if bool(kr["insert"]) != (name == "inserting") or not kr["ok"]:
            raise SystemExit("configuration %s does not do what its name says: %s" % (name, kr))
        t_res, t_host, t_glue, t_copy, t_stage = [], [], [], [], {s: [] for s in LAUNCHES}
        for _ in range(a.repeats):                                # interleaved: the machine's other work hits all alike
            t_copy.append(batch(restore))
            t_res.append(batch(resident))
            glue[0] = 0.0
            t_host.append(batch(host_driven))
            t_glue.append(glue[0] * 1e3 / a.iters)
            for s in LAUNCHES:                                    # after a composite call: *result holds the gates the later stages read
                resident()
                t_stage[s].append(batch(lambda: (restore(), stage(s))) - t_copy[-1])
        res[name] = dict(n_new=int(kr["n_new"]), n_candidates=int(kr["n_candidates"]), n_processed=int(kr["n_processed"]), n_valid=int(kr["n_valid"]),
                         resident_ms=med(t_res), resident_min_max_ms=span(t_res), host_driven_ms=med(t_host), host_driven_min_max_ms=span(t_host),
                         host_glue_ms=med(t_glue), restore_copy_ms=med(t_copy), stage_ms={s: med(v) for s, v in t_stage.items()})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
