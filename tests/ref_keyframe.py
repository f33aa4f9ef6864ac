"""Restatement of what Tracking::_Track_ does with a frame after the two track functions (hs_keyframe_*_device / hs_track_keyframe_device,
include/hyslam_amd.h), twice:

  literal(c)   the reference's own control flow on LandMarkMatches with its two std::maps (ref_track.MapMatches): determineReferenceKeyFrame
               (src/main/Tracking.cpp:273-317), bOK (TrackingStateNormal.cpp:41,71,78-82), HandlePostTrackingSuccess (Tracking.cpp:375-388),
               needNewKeyFrame (TrackingStateNormal.cpp:87-170) with KeyFrame::TrackedMapPoints (KeyFrame.cc:201-222), createNewKeyFrame with its
               sequential depth loop and `break` (TrackingState.cpp:20-93), the final outlier removal (Tracking.cpp:219-225)
  dense(c)     the kernels' algorithm on the device layout (kernels_keyframe.hip): gates as flags, the depth walk as a closed form on sorted keys;
               `mut` switches on one of the mutations tests/test_keyframe_ref.py must catch

Both return the same dict (see _pack).  A case `c` (tests/keyframe_cases.py): state = (kp_lm, kp_outl, n_matches), T (the observation table),
K (n_kf, kf_off, kp_lm: the key frames' associations), depth, frame (fx, fy, cx, cy, sensor, kps, desc), Tcw, track (status, n_matches_map,
n_inliers), prm (see PARAMS), ref_slot, new_cap.  Landmarks and key frames are indices; new landmarks are numbered L + k in
creation order (D16)."""
import numpy as np

import ref_kfgraph as RK
import ref_track as R

f32 = np.float32
# hs_keyframe_params with the reference's defaults (Tracking_datastructs.h:103-113)
PARAMS = dict(frame_id=0, last_keyframe_id=0, force=0, mapping_stopped=0, mapping_idle=1, mapping_queue_length=0, n_kfs_in_map=3, min_N_tracked_close=100,
              thresh_N_nontracked_close=70, min_KF_interval=0, max_KF_interval=30, N_tracked_target=200, N_tracked_variance=50, th_depth=40.0, n_min_points=100,
              thresh_init=10, thresh_refine=30, force_loss=0, ok_override=-1)
RESULT_KEYS = ("ok", "ref_slot", "n_valid", "n_ref_matches", "n_tracked_close", "n_nontracked_close", "insert", "n_new", "n_candidates", "n_processed")
MUTATIONS = ("ge_th", "tie_desc", "overwrite_stale", "no_max", "outlier_tracked")


def params(**kw):
    assert set(kw) <= set(PARAMS), set(kw) - set(PARAMS)
    return dict(PARAMS, **kw)


def gate(track, p):
    if p["ok_override"] >= 0:
        return int(p["ok_override"] != 0)
    return int(track["status"] == R.TRACK_OK and track["n_matches_map"] > p["thresh_init"] and track["n_inliers"] > p["thresh_refine"] and not p["force_loss"])


def unproject_stereo(u, v, z, fr, pv):
    """Frame::UnprojectStereo: Camera::Unproject in float as written, then mRwc * x3Dc + mOw as one cv::gemm (double products summed left to right
    from 0, + Ow in double, one rounding); mRwc = Rcw^T"""
    with np.errstate(all="ignore"):
        u, v, z = f32(u), f32(v), f32(z)
        x = f32(f32(u - f32(fr["cx"])) * f32(z / f32(fr["fx"])))
        y = f32(f32(v - f32(fr["cy"])) * f32(z / f32(fr["fy"])))
        Rcw, Ow = pv["Rcw"].reshape(3, 3), pv["Ow"]
        out = np.zeros(3, f32)
        for r in range(3):
            s = 0.0
            s = s + float(Rcw[0, r]) * float(x)
            s = s + float(Rcw[1, r]) * float(y)
            s = s + float(Rcw[2, r]) * float(z)
            out[r] = f32(s + float(Ow[r]))
    return out


def unproject_stereo_batch(u, v, z, fr, pv):
    """unproject_stereo on arrays, the same roundings: float32 elementwise for the camera step, float64 for the products and sums"""
    with np.errstate(all="ignore"):
        u, v, z = np.asarray(u, f32), np.asarray(v, f32), np.asarray(z, f32)
        x = (u - f32(fr["cx"])) * (z / f32(fr["fx"]))
        y = (v - f32(fr["cy"])) * (z / f32(fr["fy"]))
        Rcw, Ow = pv["Rcw"].reshape(3, 3).astype(np.float64), pv["Ow"].astype(np.float64)
        x, y, z = x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)
        out = np.empty((len(x), 3), f32)
        for r in range(3):
            out[:, r] = ((((0.0 + Rcw[0, r] * x) + Rcw[1, r] * y) + Rcw[2, r] * z) + Ow[r]).astype(f32)
    return out


def decision(p, sensor, n_tracked, n_other, inliers):
    """needNewKeyFrame's boolean, in the reference's integer types: mnId is long unsigned (64 bits), last_keyframe_id unsigned int, the intervals
    int -> the sum wraps in 32 bits and is widened for the comparison"""
    if not p["force"] and p["mapping_stopped"]:
        return 0
    need_close = n_tracked < p["min_N_tracked_close"] and n_other > p["thresh_N_nontracked_close"]
    u32 = lambda v: int(v) & 0xFFFFFFFF
    max_exceeded = int(p["frame_id"]) >= u32(u32(p["last_keyframe_id"]) + u32(p["max_KF_interval"]))
    min_exceeded = int(p["frame_id"]) >= u32(u32(p["last_keyframe_id"]) + u32(p["min_KF_interval"]))
    lack_close = sensor != 0 and need_close
    weak = inliers < p["N_tracked_target"] - p["N_tracked_variance"]
    dire = inliers < p["N_tracked_target"] - 2 * p["N_tracked_variance"]
    definite = p["force"] or max_exceeded or dire
    optional = min_exceeded and (weak or lack_close)
    insert = False
    if definite or (optional and p["mapping_idle"]):
        if p["mapping_idle"] or p["force"]:
            insert = True
        else:
            insert = p["mapping_queue_length"] < 3
    return int(bool(insert))


def _lm_obs(c, kp_lm, new_view, stage1):
    """kp_lm_obs as the kernels leave it: lm_nobs for an index in [0, L), -1 without a landmark; a provisional index (>= L) reads 0 on the views this
    call created, and on the others -1 when stage 1 (k_frame_views) rewrote the array, else what the case carried in (`kp_lm_obs`, default -1)"""
    kp_lm, L, lm_nobs = np.asarray(kp_lm), len(c["T"]["lm_nobs"]), np.asarray(c["T"]["lm_nobs"])
    inside = (kp_lm >= 0) & (kp_lm < L)
    carried = np.full(len(kp_lm), -1, np.int32) if stage1 or c.get("kp_lm_obs") is None else np.asarray(c["kp_lm_obs"], np.int32)
    out = np.where(inside, lm_nobs[np.where(inside, kp_lm, 0)] if L else -1, np.where(kp_lm >= L, carried, -1)).astype(np.int32)
    made = np.asarray(new_view, np.int64).reshape(-1)
    out[made[kp_lm[made] >= L]] = 0
    return out


def _pack(c, res, state, new_view, new_pos, pv, stage1=True):
    """the common result: `result` (RESULT_KEYS), kp_lm / kp_outl / n_matches / kp_lm_obs, pose_view, new_view / new_pos (every created point, untruncated)
    and the creation records of the first min(n_new, new_cap)"""
    L, fr, cap = len(c["T"]["lm_nobs"]), c["frame"], c["new_cap"]
    kp_lm, kp_outl, nm = state
    out = dict(result={k: int(res[k]) for k in RESULT_KEYS}, kp_lm=np.asarray(kp_lm, np.int32), kp_outl=np.asarray(kp_outl, np.uint8), n_matches=int(nm),
               kp_lm_obs=_lm_obs(c, kp_lm, new_view, stage1), pose_view=pv, new_view=np.asarray(new_view, np.int32).reshape(-1),
               new_pos=np.asarray(new_pos, f32).reshape(-1, 3))
    m = min(len(out["new_view"]), cap)
    v = out["new_view"][:m]
    ent, obs = np.zeros(m, ENTRY_DTYPE), np.zeros(m, OBS_DTYPE)
    ent["pos"], ent["ref_Ow"] = out["new_pos"][:m], pv["Ow"]
    obs["Ow"], obs["fx"], obs["fy"], obs["cx"], obs["cy"] = pv["Ow"], fr["fx"], fr["fy"], fr["cx"], fr["cy"]
    obs["u"], obs["v"], obs["kp_size"], obs["assoc_pos"], obs["assoc"] = fr["kps"]["x"][v], fr["kps"]["y"][v], fr["kps"]["size"][v], out["new_pos"][:m], 1
    lm_index = np.full(cap, -1, np.int32)
    lm_index[:m] = L + np.arange(m)
    out.update(entries=ent, obs=obs, offsets=np.arange(cap + 1, dtype=np.int64), desc=np.asarray(fr["desc"], np.uint8)[v].reshape(m, 32), lm_index=lm_index)
    return out


ENTRY_DTYPE = np.dtype([("pos", "<f4", 3), ("ref_Ow", "<f4", 3)])
OBS_DTYPE = np.dtype([("Ow", "<f4", 3), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("u", "<f4"), ("v", "<f4"), ("kp_size", "<f4"),
                      ("assoc_pos", "<f4", 3), ("assoc", "<i4")])


# ---------------------------------------------------------------- the reference, literally
def literal(c, stages=range(1, 7), res=None):
    """`stages`: which of 1 .. 6 run (a single stage's entry point); `res`: the result fields the skipped stages would have left"""
    T, K, p, fr = c["T"], c["K"], c["prm"], c["frame"]
    L, n, depth = len(T["lm_nobs"]), len(c["depth"]), np.asarray(c["depth"], f32)
    m = R.MapMatches.from_dense(*c["state"])
    res = dict(res or {k: 0 for k in RESULT_KEYS})
    pv = R.pose_view(c["Tcw"])
    new_view, new_pos = [], []
    nobs = lambda lm: int(T["lm_nobs"][lm]) if lm < L else 0
    if 1 in stages:                                             # determineReferenceKeyFrame
        counter = {}
        for i, lm in m.items():
            if lm < L and not T["lm_bad"][lm]:
                for j in range(int(T["lm_obs_offsets"][lm]), int(T["lm_obs_offsets"][lm + 1])):
                    s = int(T["lm_obs_kf"][j])
                    counter[s] = counter.get(s, 0) + 1
            elif lm < L:
                m.remove(i)
        best, mx = None, 0
        for s in sorted(counter):
            if T["kf_bad"][s]:
                continue
            if counter[s] > mx:
                mx, best = counter[s], s
        res["ref_slot"] = c["ref_slot"] if best is None else best           # `if (mCurrentFrame.mpReferenceKF)` (:181-183)
    else:
        res["ref_slot"] = c["ref_slot"]
    if 2 in stages:
        res["ok"] = gate(c["track"], p)
    ok = res["ok"]
    if 3 in stages:                                             # HandlePostTrackingSuccess
        res["n_valid"] = 0
        if ok:
            for i, lm in m.items():
                if lm < L and nobs(lm) < 1:
                    m.set_outlier(i, False)
                    m.remove(i)
            res["n_valid"] = sum(1 for i, _ in m.items() if not m.is_outlier(i))
    if 4 in stages:                                             # needNewKeyFrame
        res.update(n_ref_matches=0, n_tracked_close=0, n_nontracked_close=0, insert=0)
        if ok:
            min_obs = 2 if p["n_kfs_in_map"] <= 2 else 3
            s = res["ref_slot"]
            if 0 <= s < K["n_kf"]:                              # D15
                for j in range(int(K["kf_off"][s]), int(K["kf_off"][s + 1])):
                    lm = int(K["kp_lm"][j])
                    if lm < 0 or lm >= L:
                        continue
                    if not T["lm_bad"][lm] and T["lm_nobs"][lm] >= min_obs:
                        res["n_ref_matches"] += 1
            if fr["sensor"] != 0:
                for i in range(n):
                    if depth[i] > 0 and depth[i] < f32(p["th_depth"]):
                        if m.has(i) is not None and not m.is_outlier(i):
                            res["n_tracked_close"] += 1
                        else:
                            res["n_nontracked_close"] += 1
            res["insert"] = decision(p, fr["sensor"], res["n_tracked_close"], res["n_nontracked_close"], c["track"]["n_inliers"])
    if 5 in stages:                                             # createNewKeyFrame
        res.update(n_new=0, n_candidates=0, n_processed=0)
        if ok and res["insert"] and fr["sensor"] != 0:
            vd = [(depth[i], i) for i in range(n) if depth[i] > 0]
            vd.sort()
            res["n_candidates"] = len(vd)
            n_points = 0
            for j, (z, i) in enumerate(vd):
                create = False
                lm = m.has(i)
                if lm is None:
                    create = True
                elif nobs(lm) < 1 and lm < L:
                    create = True
                    m.remove(i)
                if create:
                    new_view.append(i)
                    new_pos.append(unproject_stereo(fr["kps"]["x"][i], fr["kps"]["y"][i], z, fr, pv))
                    m.associate(i, L + res["n_new"], False)
                    res["n_new"] += 1
                    n_points += 1
                else:
                    n_points += 1
                res["n_processed"] = j + 1
                if z > f32(p["th_depth"]) and n_points > p["n_min_points"]:
                    break
    if 6 in stages and ok:                                      # the final outlier removal
        for i, _ in m.items():
            if m.is_outlier(i):
                m.remove(i)
    return _pack(c, res, m.dense(n), new_view, new_pos, pv, 1 in stages)


# ---------------------------------------------------------------- the kernels' algorithm
def dense(c, mut=None, stages=range(1, 7), res=None):
    assert mut is None or mut in MUTATIONS
    T, K, p, fr = c["T"], c["K"], c["prm"], c["frame"]
    L, n, depth = len(T["lm_nobs"]), len(c["depth"]), np.asarray(c["depth"], f32)
    kp_lm, kp_outl, nm = np.array(c["state"][0], np.int32), np.array(c["state"][1], np.uint8), int(c["state"][2])
    lm_nobs, lm_bad = np.asarray(T["lm_nobs"], np.int64), np.asarray(T["lm_bad"])
    res = dict(res or {k: 0 for k in RESULT_KEYS})
    pv = R.pose_view(c["Tcw"])
    new_view, new_pos = [], []
    inside = lambda: (kp_lm >= 0) & (kp_lm < L)
    at = lambda a: a[np.where(inside(), kp_lm, 0)] if L else np.zeros(n, a.dtype)

    def remove(mask):
        nonlocal nm
        kp_lm[mask], kp_outl[mask] = -1, 0
        nm -= int(mask.sum())
    res["ref_slot"] = c["ref_slot"]
    if 1 in stages:                                             # k_frame_views(drop_bad), k_kf_votes, k_kfd_ref_update
        remove(inside() & (at(lm_bad) != 0))
        held = kp_lm[inside()]
        w = RK.votes_fast(T, np.array([0, len(held)], np.int64), held, None, 1, 0, 0)
        if w["max_slot"][0] >= 0:
            res["ref_slot"] = int(w["max_slot"][0])
    if 2 in stages:
        res["ok"] = gate(c["track"], p)
    ok = res["ok"]
    if 3 in stages:                                             # k_kfd_clean
        res["n_valid"] = 0
        if ok:
            remove(inside() & (at(lm_nobs) < 1))
            res["n_valid"] = int(((kp_lm >= 0) & (kp_outl != 2)).sum())
    with np.errstate(invalid="ignore"):
        th = f32(p["th_depth"])
        if 4 in stages:                                         # k_kfd_need
            res.update(n_ref_matches=0, n_tracked_close=0, n_nontracked_close=0, insert=0)
            if ok:
                s = res["ref_slot"]
                if 0 <= s < K["n_kf"]:
                    q = np.asarray(K["kp_lm"][int(K["kf_off"][s]):int(K["kf_off"][s + 1])], np.int64)
                    q = q[(q >= 0) & (q < L)]
                    res["n_ref_matches"] = int(((lm_bad[q] == 0) & (lm_nobs[q] >= (2 if p["n_kfs_in_map"] <= 2 else 3))).sum())
                if fr["sensor"] != 0:
                    close = (depth > 0) & (depth < th)
                    tracked = close & (kp_lm >= 0) & ((kp_outl != 2) | (mut == "outlier_tracked"))
                    res["n_tracked_close"], res["n_nontracked_close"] = int(tracked.sum()), int((close & ~tracked).sum())
                res["insert"] = decision(p, fr["sensor"], res["n_tracked_close"], res["n_nontracked_close"], c["track"]["n_inliers"])
        if 5 in stages:                                         # k_kfd_create_keys, k_kfd_create_rank
            res.update(n_new=0, n_candidates=0, n_processed=0)
            if ok and res["insert"] and fr["sensor"] != 0:
                cand = depth > 0
                creates = cand & ((kp_lm < 0) | (inside() & (at(lm_nobs) < 1)))
                idx = np.arange(n, dtype=np.uint64)
                keys = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ((idx if mut != "tie_desc" else np.uint64(n - 1) - idx) << np.uint64(1)) | creates.astype(np.uint64)
                n_cand = int(cand.sum())
                f = int((cand & ~((depth >= th) if mut == "ge_th" else (depth > th))).sum())
                j = f if mut == "no_max" else max(int(p["n_min_points"]), f)
                n_proc = j + 1 if (f < n_cand and j < n_cand) else n_cand
                order = np.nonzero(cand)[0][np.argsort(keys[cand], kind="stable")]          # the keys are unique
                made = order[:n_proc][creates[order[:n_proc]]]
                was_empty = kp_lm[made] < 0
                kp_lm[made] = L + np.arange(len(made))
                kp_outl[made] = np.where(~was_empty | (kp_outl[made] == 0) | (mut == "overwrite_stale"), 1, kp_outl[made])
                nm += int(was_empty.sum())
                new_view = made
                new_pos = unproject_stereo_batch(fr["kps"]["x"][made], fr["kps"]["y"][made], depth[made], fr, pv)
                res.update(n_new=len(made), n_candidates=n_cand, n_processed=n_proc)
    if 6 in stages and ok:                                      # k_kfd_discard
        remove((kp_lm >= 0) & (kp_outl == 2))
    return _pack(c, res, (kp_lm, kp_outl, nm), new_view, new_pos, pv, 1 in stages)


def same(a, b):
    """-> None when the two results agree in every field (floats bit for bit), else the name of the first that differs"""
    if a["result"] != b["result"]:
        return "result: %s" % {k: (a["result"][k], b["result"][k]) for k in RESULT_KEYS if a["result"][k] != b["result"][k]}
    for k in ("kp_lm", "kp_outl", "n_matches", "kp_lm_obs", "pose_view", "new_view", "new_pos", "entries", "obs", "offsets", "desc", "lm_index"):
        if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes() or np.asarray(a[k]).shape != np.asarray(b[k]).shape:
            return k
    return None
