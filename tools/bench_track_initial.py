#!/usr/bin/env python3
"""Times one frame of TrackingStateNormal (initialPoseEstimation + TrackLocalMap) on one MI355X, two ways, in the same process and interleaved, for
two kinds of frame; reported, not gated:

  resident      hs_track_normal_device: the motion model, the fall-back with both gates on the device, the local map and the record for the key-frame
                stage enqueued on one stream; the host reads nothing in between.  The vocabulary transform and the BoW search run on every frame.
  host_gated    the same build's public calls with the host taking the two decisions: hs_track_motion_model_device, a synchronise and a read of its
                result (32 bytes); only when the fall-back is due hs_bow_transform_device and hs_search_by_bow_kf_device, a synchronise and a read of
                the count (4 bytes), then hs_frame_associate_views_device, hs_pose_views_device, hs_pose_edges_device, hs_pose_optimize_device,
                hs_track_discard_device; then hs_track_local_map_device from the pose the frame holds.

  frame "skipped"    the motion model suffices (StateNormalParameters::thresh_init = 10): the stage reports HS_REFKF_SKIPPED
  frame "fallback"   the same inputs with thresh_init one above the motion model's return value: the fall-back runs and optimises

`refkf_skipped_alone_ms` is hs_track_reference_keyframe_device by itself on a frame that does not need it: what the always-enqueued stage costs.
Shapes: tools/bench_refkf_search.py's and tools/bench_track_frame.py's: 2 000 key points, a last frame of 1 100, 50 000 landmarks, a key frame of 2 000
in a store of 300, a synthetic 10-ary vocabulary of 4 levels with the feature vector at level 2.  Times are wall clock around a stream synchronise over
`--iters` back-to-back frames, median of `--repeats` alternating batches, smallest and largest beside it.  Both paths must leave the same associations,
counts and poses.  Prints one JSON line.
usage: bench_track_initial.py [--iters 100] [--repeats 7] [--keypoints 2000] [--landmarks 50000] [--key-frames 300]"""
import argparse
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
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--landmarks", type=int, default=50000)
    ap.add_argument("--key-frames", type=int, default=300)
    a = ap.parse_args()
    import hyslam_amd as HS
    from hyslam_amd import _native as N
    from hyslam_amd.distributed import DeviceVocabulary
    from hyslam_amd.features import _DevBuf
    from hyslam_amd.synth import synth_vocab_tree
    import scenes
    import track_cases as TC

    n, L, n_kf, levelsup = a.keypoints, a.landmarks, a.key_frames, 2
    c = TC.build(2024, n=n, n_last=min(n, 1100), extra=L - n, n_kf=n_kf, max_obs=16)
    fr, tp, T = c["frame"], c["tp"], c["T"]
    n_last, cap, per, slot = len(c["last_kp_lm"]), L, n, n_kf // 2
    rng = np.random.default_rng(2025)
    tree, tkeep, _ = synth_vocab_tree(10, 4, 17)
    ex = HS.ORBExtractor(device=0)
    tr, voc = HS.FrameTracker(ex), DeviceVocabulary(ex, tree, levelsup, keepalive=tkeep)
    # the store: key frame `slot` sees seven tenths of the frame's points under a camera turned by 25 degrees, each on one view
    total = per * n_kf
    K = dict(n_kf=n_kf, kf_off=(np.arange(n_kf + 1) * per).astype(np.int64), kps=np.zeros(total, N.KP_DTYPE), desc=rng.integers(0, 256, (total, 32), dtype=np.uint8),
             kp_lm=np.where(rng.random(total) < 0.6, rng.integers(0, L, total), -1).astype(np.int32))
    src, lo = rng.permutation(n), slot * per
    K["desc"][lo:lo + per] = scenes.flip_bits(rng, fr["desc"][src], rng.integers(0, 12, per))
    K["kps"]["angle"][lo:lo + per] = ((fr["kps"]["angle"][src] + 25 + rng.normal(0, 3, per)) % 360).astype(np.float32)
    K["kp_lm"][lo:lo + per] = np.where(rng.random(per) < 0.7, c["slot"][src], -1)
    Tl = c["Tcw_pred"].copy()
    Tl[:3, 3] += np.array([0.02, -0.01, 0.015], np.float32)       # the last frame's pose, from which the fall-back optimises

    up = lambda x: _DevBuf(ex, np.ascontiguousarray(x).nbytes, np.ascontiguousarray(x))
    F, fkeep = tr.device_frame(fr)
    KT, tabkeep = tr.device_table(T)
    lms = np.ascontiguousarray(c["lms"], N.LM_DTYPE)
    d_lms, d_Tp, d_Tl, d_lk, d_ll = up(lms), up(c["Tcw_pred"]), up(Tl), up(np.ascontiguousarray(c["last_kps"], N.KP_DTYPE)), up(c["last_kp_lm"])
    d_ng, d_pa, d_slot = up(c["neigh"]), up(c["parent"]), up(np.array([slot], np.int32))
    kbufs = [up(K["kf_off"]), up(K["kps"]), up(K["desc"]), up(K["kp_lm"])]
    k_word, k_weight, k_node = (_DevBuf(ex, total * 4) for _ in range(3))
    voc.transform_device(kbufs[2].ptr, 0, total, k_word.ptr, k_weight.ptr, k_node.ptr)        # the store's nodes and weights as the transform leaves them
    ex.synchronize()
    KF = N.KfFeatures(n_kf, kbufs[0].ptr, kbufs[1].ptr, kbufs[2].ptr, k_node.ptr, kbufs[3].ptr, k_weight.ptr)
    st = [_DevBuf(ex, n * 4), _DevBuf(ex, n), _DevBuf(ex, 4), _DevBuf(ex, n * 4)]              # the motion model clears the state: every frame starts alike
    ST = N.TrackState(*[b.ptr for b in st])
    out, ob = tr.outputs(dict(n=n, n_last=n_last, n_kf=n_kf, cap=cap))
    iout, ib = tr.initial_outputs(n, per)
    work = _DevBuf(ex, tr.track_initial_work_bytes(n, n_last, L, cap, per))
    prm = N.TrackParams(tp.th_motion, tp.th_motion_wide, tp.n_min_matches, tp.th_local, tp.nnratio_motion, tp.nnratio_local, tp.th_high, tp.sigma_ref,
                        tp.n_max_local_keyframes, tp.n_neighbor_keyframes)
    rd = lambda bufs, k: bufs[k][0].read(bufs[k][1], bufs[k][2])
    neigh_cap = c["neigh"].shape[1]
    off_tcw = N.POSE_RESULT_DTYPE.fields["Tcw"][1]
    off_nbow, off_map = (N.TRACK_INITIAL_RESULT_DTYPE.fields[k][1] for k in ("n_bow", "n_matches_map_refkf"))

    def resident(rp):
        tr.track_normal_device(F, 1, d_Tp.ptr, d_lk.ptr, d_ll.ptr, n_last, voc._v, KF, d_slot.ptr, per, d_Tl.ptr, None, KT, d_lms.ptr, d_ng.ptr, neigh_cap, d_pa.ptr, cap,
                               prm, rp, ST, out, iout, work.ptr)

    # ---- the host-gated sequence over the same buffers
    prob = np.zeros(1, N.POSE_PROBLEM_DTYPE)                      # the fall-back's problem: the last frame's pose with the frame's camera
    prob["Tcw"][0] = Tl.ravel()
    prob["fx"], prob["fy"], prob["cx"], prob["cy"], prob["bf"] = (fr[k] for k in ("fx", "fy", "cx", "cy", "mbf"))
    d_prob = up(prob)
    Fs = N.FrameView.from_buffer_copy(F)
    Fs.kp_lm_obs = st[3].ptr
    vwork = _DevBuf(ex, tr.track_refkf_work_bytes(n, per, L))
    ran = dict(fallback=0, optimised=0)

    def host_gated(rp):
        tr.track_motion_model_device(F, d_Tp.ptr, d_lk.ptr, d_ll.ptr, n_last, KT, d_lms.ptr, prm, ST, out, work.ptr)
        ex.synchronize()
        m = rd(ob, "result")[0]                                  # the first gate word
        ret = -1 if int(m["status"]) == N.HS_TRACK_MOTION_FAILED else int(m["n_matches_map"])
        d_pose = ob["pose_motion"][0].ptr + off_tcw
        if ret < rp.thresh_init:
            ran["fallback"] += 1
            voc.transform_device(fkeep[1].ptr, 0, n, ib["bow_word"][0].ptr, ib["bow_weight"][0].ptr, ib["bow_node"][0].ptr)
            tr.search_by_bow_kf_device(KF, d_slot.ptr, KT, fkeep[0].ptr, fkeep[1].ptr, ib["bow_node"][0].ptr, ib["bow_weight"][0].ptr, n, rp.th_low, rp.nnratio,
                                       ib["match_kf"][0].ptr, per, ib["op_view"][0].ptr, ib["op_lm"][0].ptr, ib["result"][0].ptr + off_nbow)
            ex.synchronize()
            n_bow = int(ib["result"][0].read(np.int32, 1, off_nbow)[0])      # the second gate word
            if n_bow >= rp.n_min_matches_bow:
                ran["optimised"] += 1
                tr.frame_associate_views_device(n, L, st[0].ptr, st[1].ptr, st[2].ptr, ib["op_view"][0].ptr, ib["op_lm"][0].ptr, vwork.ptr)
                tr.pose_views_device(d_Tl.ptr, ib["pose_view"][0].ptr)
                ex.pose_edges_device(Fs, d_lms.ptr, L, st[0].ptr, ib["edges"][0].ptr, n, ib["n_edges"][0].ptr, tp.sigma_ref)
                ex.pose_optimize_device(1, d_prob.ptr, ib["edges"][0].ptr, ib["outlier"][0].ptr, ib["pose"][0].ptr, None, ib["n_edges"][0].ptr, n)
                tr.track_discard_device(N.HS_TRACK_MOTION, ib["edges"][0].ptr, ib["n_edges"][0].ptr, n, ib["outlier"][0].ptr, ib["pose"][0].ptr, KT, fr["sensor"], st[0].ptr,
                                        st[1].ptr, st[2].ptr, ib["result"][0].ptr + off_map)
                d_pose = ib["pose"][0].ptr + off_tcw
        tr.track_local_map_device(F, d_pose, KT, d_lms.ptr, d_ng.ptr, neigh_cap, d_pa.ptr, cap, prm, ST, out, work.ptr)

    def snapshot():
        ex.synchronize()
        return (st[0].read(np.int32, n).tobytes(), st[1].read(np.uint8, n).tobytes(), int(st[2].read(np.int32, 1)[0]), int(rd(ob, "result")[0]["n_inliers"]),
                rd(ob, "pose_local")[0].tobytes())

    def batch(call):
        ex.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            call()
        ex.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.iters

    med = lambda v: round(float(np.median(v)), 4)
    span = lambda v: [round(float(min(v)), 4), round(float(max(v)), 4)]
    resident(N.TrackRefkfParams()); ex.synchronize()
    n_map = int(rd(ob, "result")[0]["n_matches_map"])
    frames = dict(skipped=N.TrackRefkfParams(thresh_init=10), fallback=N.TrackRefkfParams(thresh_init=n_map + 1))
    res = dict(keypoints=n, last_frame_keypoints=n_last, landmarks=L, key_frames=n_kf, keyframe_keypoints=per, iters=a.iters, repeats=a.repeats, motion_n_matches_map=n_map)
    for kind, rp in frames.items():
        resident(rp)
        want = snapshot()
        r = rd(ib, "result")[0]
        ran.update(fallback=0, optimised=0)
        host_gated(rp)
        if snapshot() != want:
            raise SystemExit("%s: the resident call and the host-gated sequence disagree" % kind)
        status = int(r["refkf_status"])
        if (kind == "skipped") != (status == N.HS_REFKF_SKIPPED) or (kind == "fallback" and (status != N.HS_REFKF_OK or ran["optimised"] != 1)):
            raise SystemExit("%s: the scene does not make this kind of frame (status %d)" % (kind, status))
        batch(lambda: resident(rp)); batch(lambda: host_gated(rp))            # warm-up
        t_res, t_host = [], []
        for _ in range(a.repeats):                                # interleaved: the machine's other work hits both alike
            t_res.append(batch(lambda: resident(rp)))
            t_host.append(batch(lambda: host_gated(rp)))
        res[kind] = dict(refkf_status=status, n_bow=int(r["n_bow"]), n_init=int(r["n_init"]), success=int(r["success"]), n_inliers=want[3], resident_ms=med(t_res),
                         resident_min_max_ms=span(t_res), host_gated_ms=med(t_host), host_gated_min_max_ms=span(t_host))
    # what the always-enqueued stage costs a frame that did not need it: the call by itself, predicated on a motion result that suffices
    rp = frames["skipped"]
    resident(rp); ex.synchronize()
    alone = lambda: tr.track_reference_keyframe_device(F, voc._v, KF, d_slot.ptr, per, d_Tl.ptr, ob["pose_motion"][0].ptr + off_tcw, ob["result"][0].ptr, KT, d_lms.ptr, prm,
                                                       rp, ST, iout, work.ptr)
    batch(alone)
    res["refkf_skipped_alone_ms"] = med([batch(alone) for _ in range(a.repeats)])
    if int(rd(ib, "result")[0]["refkf_status"]) != N.HS_REFKF_SKIPPED:
        raise SystemExit("the stage alone did not skip")
    print(json.dumps(res))
    del tabkeep


if __name__ == "__main__":
    main()
