"""Restatement of the tracker's first stage with its fall-back (TrackReferenceKeyFrame::track, TrackingStateNormal::initialPoseEstimation), twice:

  LITERAL  search_by_bow_kf, associate_landmarks, track_reference_keyframe, initial_pose_estimation, track_normal: the reference's text
           (FeatureMatcher.cc:216-278, Frame.cc:221-232, TrackReferenceKeyFrame.cpp:10-58, TrackingStateNormal.cpp:21-58) with Python dicts walked as
           the std::maps, ref_track.MapMatches for LandMarkMatches, ref_bow.search_by_bow over ref_bow.feature_vector for the node walk
  DENSE    search_by_bow_kf_dense, replay_views_closed_form: hs_search_by_bow_kf_device and hs_frame_associate_views_device (include/hyslam_amd.h,
           DESIGN.md 5.13) computed the way the kernels do; reference_keyframe_dense, initial_pose_dense, track_normal_dense: the whole stage chained
           from them and the existing device calls' restatements, with the gates as dense flags (DESIGN.md 5.13 "the chain"): what a resident
           composite has to reproduce field by field

tests/test_refkf_ref.py proves the two equal on every case, and the closed form of the replay exhaustively against the sequential loop.
Landmarks and key frames are indices in ascending address order."""
import numpy as np

import ref_bow
import ref_track as R

f32 = np.float32
NONE = 0x7FFFFFFF
REFKF_OK, REFKF_BOW_FAILED, REFKF_SKIPPED = 0, 1, 2
INIT_RESULT_DTYPE = np.dtype([("refkf_status", "<i4"), ("n_bow", "<i4"), ("n_matches_map_refkf", "<i4"), ("n_init", "<i4"), ("success", "<i4"), ("_pad", "<i4", 3)])


class RefKfParams:
    def __init__(self, th_low=50.0, nnratio=0.7, n_min_matches_bow=15, thresh_init=10):
        self.th_low, self.nnratio, self.n_min_matches_bow, self.thresh_init = th_low, nnratio, n_min_matches_bow, thresh_init


# ---------------------------------------------------------------- the key-frame store
def keyframe_of(K, slot, kf_cap):
    """the keypoints of key frame `slot` as (kps, desc, node, kp_lm), truncated to kf_cap in ascending index; nothing for a slot outside the store"""
    if not 0 <= slot < K["n_kf"]:
        a = b = 0
    else:
        a, b = int(K["kf_off"][slot]), int(K["kf_off"][slot + 1])
        b = min(b, a + kf_cap)
    return K["kps"][a:b], K["desc"][a:b], K["node"][a:b], K["kp_lm"][a:b]


def frame_nodes(tree, levelsup, desc):
    """Frame::ComputeBoW -> (word, weight, node) per keypoint: hs_bow_transform_device's three outputs"""
    return ref_bow.bow_transform(tree, desc, levelsup)


# ---------------------------------------------------------------- LITERAL
def search_by_bow_kf(K, slot, kf_cap, lm_bad, fkps, fdesc, fword, fweight, fnode, th_low, nnratio):
    """FeatureMatcher::SearchByBoW(KeyFrame*, Frame&, map&) -> (matches {idx_f: lm}, matches_internal {idx_kf: idx_f}, its size)"""
    kk, kd, knode, klm = keyframe_of(K, slot, kf_cap)
    fv_kf = ref_bow.feature_vector(np.zeros(len(knode), np.int32), (np.asarray(knode) >= 0).astype(f32), knode)      # a negative node: not in mFeatVec
    fv_f = ref_bow.feature_vector(fword, fweight, fnode)
    keep1 = np.array([lm >= 0 and not lm_bad[lm] for lm in klm], np.uint8)                                            # PreviouslyMatchedIndexCriterion(true)
    match12, n = ref_bow.search_by_bow(kk, kd, fv_kf, fkps, fdesc, fv_f, keep1, th_low, nnratio, True)
    internal = {int(i): int(match12[i]) for i in np.nonzero(match12 >= 0)[0]}
    matches = {}
    for idx_kf in sorted(internal):                                  # :269-274: the later key-frame index overwrites
        matches[internal[idx_kf]] = int(klm[idx_kf])
    assert n == len(internal)
    return matches, internal, n


def associate_landmarks(matches, associations):
    """Frame::associateLandMarks(associations, true): the std::map<size_t, MapPoint*> in key order"""
    for idx in sorted(associations):
        matches.associate(int(idx), int(associations[idx]), True)
    return matches


def track_reference_keyframe(c, matches, slot=None, kf_cap=None):
    """TrackReferenceKeyFrame::track -> dict; `matches` (MapMatches or DenseMatches) is the frame's LandMarkMatches, updated in place.
    ret = the return value (-1: the BoW gate); pose = the optimiser's result, None when the gate failed"""
    fr, rp, T = c["frame"], c["rp"], c["T"]
    n = len(fr["kps"])
    slot = c["kf_slot"] if slot is None else slot
    kf_cap = c["kf_cap"] if kf_cap is None else kf_cap
    word, weight, node = frame_nodes(c["tree"], c["levelsup"], fr["desc"])
    bow, internal, nmatches = search_by_bow_kf(c["K"], slot, kf_cap, T["lm_bad"], fr["kps"], fr["desc"], word, weight, node, rp.th_low, rp.nnratio)
    out = dict(matches_bow=bow, internal=internal, n_bow=nmatches, ret=-1, pose=None)
    if nmatches < rp.n_min_matches_bow:
        out["state"] = matches.dense(n)
        return out
    associate_landmarks(matches, bow)
    out["after_associate"] = matches.dense(n)
    out["edges"], out["n_edges"], out["pose"], out["cam"] = R.optimize(fr, c["Tcw_last"], matches, c["lms"], c["tp"])
    out["ret"] = R.discard(matches, R.MOTION, fr["sensor"], T["lm_nobs"])
    out["state"] = matches.dense(n)
    return out


def initial_pose_estimation(c, velocity_valid, matches):
    """TrackingStateNormal::initialPoseEstimation -> dict(motion, refkf, n_init, success, Tcw): Tcw = the pose the frame holds afterwards (the
    caller's Tcw_entry where the reference's frame was never given one)"""
    fr, rp = c["frame"], c["rp"]
    motion = refkf = None
    if not velocity_valid:
        Tcw = np.asarray(c["Tcw_entry"], f32)
        refkf = track_reference_keyframe(c, matches)
        nmatches = refkf["ret"]
    else:
        motion = R.track_motion_model(fr, c["Tcw_pred"], c["last_kps"], c["last_kp_lm"], c["lms"], c["T"]["lm_nobs"], c["tp"], matches)
        nmatches = -1 if motion["status"] == R.TRACK_MOTION_FAILED else motion["n_matches_map"]
        Tcw = np.asarray(motion["pose"]["Tcw"], f32)
        if nmatches < rp.thresh_init:
            refkf = track_reference_keyframe(c, matches)
            nmatches = refkf["ret"]
    if refkf is not None and refkf["pose"] is not None:
        Tcw = np.asarray(refkf["pose"]["Tcw"], f32)
    return dict(motion=motion, refkf=refkf, n_init=nmatches, success=int(nmatches > rp.thresh_init), Tcw=Tcw.reshape(4, 4), state=matches.dense(len(fr["kps"])))


def track_normal(c, velocity_valid, matches, Tcw_init=None):
    """initialPoseEstimation, then TrackLocalMap::track from the pose it left (Tcw_init: the device's, when its float rounding differs)"""
    init = initial_pose_estimation(c, velocity_valid, matches)
    local = R.track_local_map(c["frame"], init["Tcw"] if Tcw_init is None else Tcw_init, c["T"], c["lms"], c["neigh"], c["parent"], c["cap"], c["tp"], matches)
    return init, local


# ---------------------------------------------------------------- DENSE
def search_by_bow_kf_dense(K, slot, kf_cap, L, lm_bad, fkps, fdesc, fnode, fweight, th_low, nnratio):
    """hs_search_by_bow_kf_device -> (match_kf [kf_cap], op_view [n], op_lm [n], n_matches): per key-frame keypoint the smallest key
    dist << 32 | frame index over the frame's keypoints of its node; the histogram; the largest key-frame index per view"""
    n = len(fkps)
    kk, kd, knode, klm = keyframe_of(K, slot, kf_cap)
    match_kf = np.full(kf_cap, -1, np.int32)
    fnode = np.asarray(fnode, np.int64)
    in_fv = np.ones(n, bool) if fweight is None else np.asarray(fweight, f32) > 0
    for j in range(len(kk)):
        lm = int(klm[j])
        if knode[j] < 0 or not 0 <= lm < L or lm_bad[lm]:
            continue
        cand = np.nonzero((fnode == knode[j]) & in_fv)[0]
        if len(cand) == 0:
            continue
        d = np.unpackbits(fdesc[cand] ^ kd[j][None, :], axis=1).sum(1).astype(np.int64)
        key = np.sort((d << 32) | cand)
        best, second = int(key[0] >> 32), (f32(key[1] >> 32) if len(key) > 1 else ref_bow.FLT_MAX)
        with np.errstate(all="ignore"):
            if f32(best) < f32(th_low) and f32(best) < f32(f32(nnratio) * second):
                match_kf[j] = int(key[0] & 0xFFFFFFFF)
    live = np.nonzero(match_kf >= 0)[0]
    if len(live):
        bins, _ = ref_bow.rotation_bins(kk["angle"][live], fkps["angle"][match_kf[live]])          # rot = frame angle - key-frame angle
        keep = [i for i in ref_bow.three_maxima(np.bincount(bins, minlength=30)) if i >= 0]
        match_kf[live[~np.isin(bins, keep)]] = -1
    live = np.nonzero(match_kf >= 0)[0]
    winner = np.full(n, -1, np.int64)
    np.maximum.at(winner, match_kf[live], live)
    op_view = np.where(winner >= 0, np.arange(n), -1).astype(np.int32)
    op_lm = np.where(winner >= 0, np.asarray(klm, np.int64)[np.maximum(winner, 0)] if len(klm) else -1, -1).astype(np.int32)
    return match_kf, op_view, op_lm, len(live)


def replay_views_sequential(matches, op_view, op_lm, n, L):
    """the ops in ascending VIEW index, one associateLandMark each"""
    ok = np.nonzero(R.valid_ops(op_view, op_lm, n, L))[0]
    for j in ok[np.argsort(np.asarray(op_view)[ok], kind="stable")]:
        matches.associate(int(op_view[j]), int(op_lm[j]), True)
    return matches


def replay_views_closed_form(kp_lm, kp_outl, n_matches, op_view, op_lm, L):
    """the kernels' phases on arrays (k_vassoc_ops, k_vassoc_holders, k_vassoc_final) -> (kp_lm, kp_outl, n_matches)"""
    kp0, outl = np.asarray(kp_lm, np.int64), np.asarray(kp_outl, np.uint8).copy()
    n = len(kp0)
    ok = R.valid_ops(op_view, op_lm, n, L)
    v, m = np.asarray(op_view, np.int64)[ok], np.asarray(op_lm, np.int64)[ok]
    view_op = np.full(n, -1, np.int64)
    lm_view = np.full(max(L, 1), NONE, np.int64)
    view_op[v], lm_view[m] = m, v
    held = (kp0 >= 0) & (kp0 < L)
    k = np.where(held, kp0, 0)
    holder = held & (lm_view[k] != NONE) & ((view_op < 0) | (np.arange(n) >= lm_view[k]))
    idx_old = np.full(max(L, 1), NONE, np.int64)
    np.minimum.at(idx_old, kp0[holder], np.nonzero(holder)[0])
    erased = held & (lm_view[k] != NONE) & (idx_old[k] == np.arange(n))
    has_op = view_op >= 0
    fresh = has_op & ((kp0 < 0) | (erased & (lm_view[k] < np.arange(n)))) & (idx_old[np.where(has_op, view_op, 0)] == NONE)
    out = np.where(has_op, view_op, np.where(erased, -1, kp0))
    outl[has_op & ~(fresh & (outl != 0))] = 1
    return out.astype(np.int32), outl, int(n_matches) + int(fresh.sum())


def _gate(motion, n_bow, rp):
    run = True if motion is None else (-1 if motion["status"] == R.TRACK_MOTION_FAILED else motion["n_matches_map"]) < rp.thresh_init
    return REFKF_SKIPPED if not run else REFKF_BOW_FAILED if n_bow < rp.n_min_matches_bow else REFKF_OK


def reference_keyframe_dense(c, state, Tcw_entry, motion=None, slot=None, kf_cap=None):
    """the stage as a chain of device calls (motion: the motion stage's result when the stage is predicated on it) -> every intermediate by name,
    `state` (kp_lm, kp_outl, n_matches) afterwards, and `cam`, `status`"""
    fr, rp, T, tp = c["frame"], c["rp"], c["T"], c["tp"]
    n, L = len(fr["kps"]), len(c["lms"])
    slot = c["kf_slot"] if slot is None else slot
    kf_cap = c["kf_cap"] if kf_cap is None else kf_cap
    word, weight, node = frame_nodes(c["tree"], c["levelsup"], fr["desc"])
    match_kf, op_view, op_lm, n_bow = search_by_bow_kf_dense(c["K"], slot, kf_cap, L, T["lm_bad"], fr["kps"], fr["desc"], node, weight, rp.th_low, rp.nnratio)
    status = _gate(motion, n_bow, rp)
    active = status == REFKF_OK
    kp_lm, kp_outl, nm = (np.asarray(state[0], np.int32).copy(), np.asarray(state[1], np.uint8).copy(), int(state[2]))
    if active:
        kp_lm, kp_outl, nm = replay_views_closed_form(kp_lm, kp_outl, nm, op_view, op_lm, L)
    m = R.DenseMatches.from_dense(kp_lm, kp_outl, nm)
    edges, n_edges, pose, cam = R.optimize(fr, c["Tcw_last"], m, c["lms"], tp, run=active)
    n_map = R.discard(m, R.MOTION, fr["sensor"], T["lm_nobs"]) if active else 0
    res = np.zeros(1, INIT_RESULT_DTYPE)
    motion_return = 0 if motion is None else (-1 if motion["status"] == R.TRACK_MOTION_FAILED else motion["n_matches_map"])
    n_init = n_map if active else -1 if status == REFKF_BOW_FAILED else motion_return
    res["refkf_status"], res["n_bow"], res["n_matches_map_refkf"], res["n_init"], res["success"] = status, n_bow, n_map, n_init, int(n_init > rp.thresh_init)
    Tcw_init = np.asarray(pose["Tcw"] if active else Tcw_entry, f32).reshape(16)
    return dict(bow_word=word, bow_weight=weight, bow_node=node, match_kf=match_kf, op_view=op_view, op_lm=op_lm, edges=edges, n_edges=[n_edges, n_edges if active else 0],
                pose=pose, Tcw_init=Tcw_init, result=res, state=m.dense(), cam=cam, status=status, after_associate=(kp_lm, kp_outl, nm))


def initial_pose_dense(c, velocity_valid, state):
    """initialPoseEstimation on the dense state -> (motion or None, refkf)"""
    fr = c["frame"]
    if not velocity_valid:
        return None, reference_keyframe_dense(c, state, c["Tcw_entry"])
    m = R.DenseMatches.from_dense(*state)
    motion = R.track_motion_model(fr, c["Tcw_pred"], c["last_kps"], c["last_kp_lm"], c["lms"], c["T"]["lm_nobs"], c["tp"], m)
    return motion, reference_keyframe_dense(c, motion["state"], motion["pose"]["Tcw"], motion)


def track_normal_dense(c, velocity_valid, state, Tcw_init=None):
    """initialPoseEstimation + TrackLocalMap on the dense state -> (motion or None, refkf, local)"""
    motion, refkf = initial_pose_dense(c, velocity_valid, state)
    T_in = (refkf["Tcw_init"] if Tcw_init is None else np.asarray(Tcw_init, f32)).reshape(4, 4)
    local = R.track_local_map(c["frame"], T_in, c["T"], c["lms"], c["neigh"], c["parent"], c["cap"], c["tp"], R.DenseMatches.from_dense(*refkf["state"]))
    return motion, refkf, local
