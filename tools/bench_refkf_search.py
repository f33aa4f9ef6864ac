#!/usr/bin/env python3
"""Times the first half of TrackReferenceKeyFrame::track (ComputeBoW, SearchByBoW(KeyFrame*, Frame&), associateLandMarks) on one MI355X, two
ways, in the same process and interleaved; reported, not gated:

  resident      hs_bow_transform_device, hs_search_by_bow_kf_device (which reads the transform's node and weight arrays as they are) and
                hs_frame_associate_views_device enqueued on one stream over a key-frame store resident in HBM; the host reads nothing in between.
  host_driven   what the library offered before: hs_bow_transform and hs_search_by_bow with host pointers (the feature vectors as CSR lists built
                on the host, the key frame's `keep` flags from the host's tables), then the association loop on the host and an upload of the state
                the next device call reads.  The host glue here is numpy; `host_glue_ms` is its share.

Shapes: a frame of 2 000 key points, a key frame of 2 000 in a store of 300 key frames, 50 000 landmarks, a synthetic 10-ary vocabulary of 4 levels
with the feature vector at level 2 (100 nodes).  Times are wall clock around a stream synchronise over `--iters` back-to-back frames, median of
`--repeats` alternating batches, smallest and largest beside it.  Both paths must leave the same associations.  Prints one JSON line.
usage: bench_refkf_search.py [--iters 100] [--repeats 7] [--keypoints 2000] [--landmarks 50000] [--key-frames 300]"""
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
    import ref_track as R
    import scenes

    n, L, n_kf, levelsup = a.keypoints, a.landmarks, a.key_frames, 2
    rng = np.random.default_rng(2025)
    tree, tkeep, _ = synth_vocab_tree(10, 4, 17)
    ex = HS.ORBExtractor(device=0)
    tr, voc, host_voc = HS.FrameTracker(ex), DeviceVocabulary(ex, tree, levelsup, keepalive=tkeep), HS.ORBVocabulary(tree, ex)
    matcher = HS.FeatureMatcher(HS.FeatureMatcherSettings(nnratio=0.7, TH_LOW=50.0), ex)
    # the frame, and a store whose key frame `slot` sees the frame's points under a turned camera
    kps = np.zeros(n, N.KP_DTYPE)
    kps["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    per, slot = n, n_kf // 2
    total = per * n_kf
    K = dict(n_kf=n_kf, kf_off=(np.arange(n_kf + 1) * per).astype(np.int64), kps=np.zeros(total, N.KP_DTYPE), desc=rng.integers(0, 256, (total, 32), dtype=np.uint8),
             kp_lm=np.where(rng.random(total) < 0.6, rng.integers(0, L, total), -1).astype(np.int32))
    src = rng.permutation(n)
    lo = slot * per
    K["desc"][lo:lo + per] = scenes.flip_bits(rng, desc[src], rng.integers(0, 12, per))
    K["kps"]["angle"][lo:lo + per] = ((kps["angle"][src] + 25 + rng.normal(0, 3, per)) % 360).astype(np.float32)
    K["kp_lm"][lo:lo + per] = np.where(rng.random(per) < 0.6, rng.permutation(L)[:per], -1)      # a key frame holds a landmark on one view
    _, _, (kw, kwt, knd) = host_voc.transform(K["desc"][lo:lo + per], levelsup)
    K["node"], K["weight"] = np.full(total, -1, np.int32), np.zeros(total, np.float32)      # the transform's outputs as they are, for the key frame in use
    K["node"][lo:lo + per], K["weight"][lo:lo + per] = knd, kwt
    table = dict(lm_obs_offsets=np.zeros(L + 1, np.int64), lm_obs_kf=np.zeros(0, np.int32), lm_obs_octave=np.zeros(0, np.int32),
                 lm_bad=(rng.random(L) < 0.02).astype(np.uint8), lm_nobs=np.ones(L, np.int32), kf_bad=np.zeros(n_kf, np.uint8), kf_id=np.arange(n_kf, dtype=np.int64))
    state0 = (np.where(rng.random(n) < 0.3, rng.integers(0, L, n), -1).astype(np.int32), rng.integers(1, 3, n).astype(np.uint8), 0)

    up = lambda x: _DevBuf(ex, np.ascontiguousarray(x).nbytes, np.ascontiguousarray(x))
    KF, kkeep = tr.device_keyframes(K)
    KT, tabkeep = tr.device_table(table)
    d_kps, d_desc, d_slot = up(kps), up(desc), up(np.array([slot], np.int32))
    d_word, d_weight, d_node = _DevBuf(ex, n * 4), _DevBuf(ex, n * 4), _DevBuf(ex, n * 4)
    d_match, d_opv, d_opl, d_nm = _DevBuf(ex, per * 4), _DevBuf(ex, n * 4), _DevBuf(ex, n * 4), _DevBuf(ex, 4)
    d_state = [up(state0[0]), up(state0[1]), up(np.array([state0[2]], np.int32))]
    work = _DevBuf(ex, tr.track_refkf_work_bytes(n, per, L))

    def resident():                                              # in the timed loop the replay runs on the state the last frame left: the same launches
        voc.transform_device(d_desc.ptr, 0, n, d_word.ptr, d_weight.ptr, d_node.ptr)
        tr.search_by_bow_kf_device(KF, d_slot.ptr, KT, d_kps.ptr, d_desc.ptr, d_node.ptr, d_weight.ptr, n, 50.0, 0.7, d_match.ptr, per, d_opv.ptr, d_opl.ptr, d_nm.ptr)
        tr.frame_associate_views_device(n, L, d_state[0].ptr, d_state[1].ptr, d_state[2].ptr, d_opv.ptr, d_opl.ptr, work.ptr)

    glue = [0.0]
    kk, kd, klm = K["kps"][lo:lo + per], K["desc"][lo:lo + per], K["kp_lm"][lo:lo + per]
    fv_kf = host_voc.transform(kd, levelsup)[1]                  # the key frame's feature vector was computed when it was made

    def host_driven():
        _, fv_f, _ = host_voc.transform(desc, levelsup)         # hs_bow_transform + the CSR lists on the host
        t0 = time.perf_counter()
        keep = ((klm >= 0) & (table["lm_bad"][np.maximum(klm, 0)] == 0)).astype(np.uint8)
        glue[0] += time.perf_counter() - t0
        m, _ = matcher.SearchByBoW(kk, kd, fv_kf, kps, desc, fv_f, keep, True)
        t0 = time.perf_counter()
        st = R.DenseMatches.from_dense(*state0)
        bow = {}
        for j in np.nonzero(m >= 0)[0]:
            bow[int(m[j])] = int(klm[j])
        for f in sorted(bow):
            st.associate(f, bow[f], True)
        glue[0] += time.perf_counter() - t0
        for d, x in zip(d_state, (st.kp_lm, st.kp_outl, np.array([st.n_matches], np.int32))):
            d.write(x)
        return st

    # both paths leave the same associations from the same entry state
    resident(); ex.synchronize()
    got = d_state[0].read(np.int32, n), d_state[1].read(np.uint8, n), int(d_state[2].read(np.int32, 1)[0])
    want = host_driven().dense()
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), "the two paths disagree"
    n_bow = int(d_nm.read(np.int32, 1)[0])

    def batch(fn):
        ex.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            fn()
        ex.synchronize()
        return (time.perf_counter() - t0) / a.iters * 1e3
    for fn in (resident, host_driven):
        batch(fn)                                                # warm-up
    times = dict(resident=[], host_driven=[])
    glue[0] = 0.0
    for _ in range(a.repeats):
        times["resident"].append(batch(resident))
        times["host_driven"].append(batch(host_driven))
    # the device time of the resident stages alone, each in its own batch
    stage = {}
    for name, fn in (("bow_transform", lambda: voc.transform_device(d_desc.ptr, 0, n, d_word.ptr, d_weight.ptr, d_node.ptr)),
                     ("search_by_bow_kf", lambda: tr.search_by_bow_kf_device(KF, d_slot.ptr, KT, d_kps.ptr, d_desc.ptr, d_node.ptr, d_weight.ptr, n, 50.0, 0.7, d_match.ptr, per,
                                                                             d_opv.ptr, d_opl.ptr, d_nm.ptr)),
                     ("associate_views", lambda: tr.frame_associate_views_device(n, L, d_state[0].ptr, d_state[1].ptr, d_state[2].ptr, d_opv.ptr, d_opl.ptr, work.ptr))):
        batch(fn)
        stage[name + "_ms"] = round(float(np.median([batch(fn) for _ in range(3)])), 4)
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps(dict(keypoints=n, keyframe_keypoints=per, landmarks=L, key_frames=n_kf, n_bow=n_bow, iters=a.iters, repeats=a.repeats,
                          resident_ms=round(med["resident"], 4), resident_min_max=[round(min(times["resident"]), 4), round(max(times["resident"]), 4)],
                          host_driven_ms=round(med["host_driven"], 4), host_driven_min_max=[round(min(times["host_driven"]), 4), round(max(times["host_driven"]), 4)],
                          host_glue_ms=round(glue[0] / (a.iters * a.repeats) * 1e3, 4), **stage)))
    del kkeep, tabkeep


if __name__ == "__main__":
    main()
