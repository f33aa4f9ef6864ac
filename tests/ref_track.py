"""Restatement of the reference's per-frame tracking for the resident chain (hs_track_*_device, include/hyslam_amd.h):

  LandMarkMatches             src/core/LandMarkMatches.cpp:6-110 — the maps, as the C++ (MapMatches), and the dense-array model of
                              hyslam_amd/host/HipAssociationReplay.h (DenseMatches); both offer the same calls, so the track functions run on either
  replay_closed_form          the numpy twin of the kernels' algorithm (kernels_track.hip): what tests/test_track_ref.py proves
                              against the sequential loop, exhaustively
  pose_view                   Frame::UpdatePoseMatrices (mOw as one cv::gemm)
  search_by_projection        FeatureMatcher::_SearchByProjection_ (FeatureMatcher.cc:57-176) on pyref's primitives, pose taken from a pose view
  track_motion_model          src/slam/tracking/TrackMotionModel.cpp:33-81
  track_local_map             src/slam/tracking/TrackLocalMap.cpp:9-78 (on ref_kfgraph / ref_localmap)

Landmarks are indices; containers the reference orders by MapPoint* are walked in ascending index."""
import numpy as np

import pyref
import ref_bow
import ref_kfgraph as RK
import ref_localmap as RL
import ref_poseopt as RP

f32 = np.float32
NONE = 0x7FFFFFFF
TRACK_OK, TRACK_MOTION_FAILED = 0, 1
MOTION, LOCAL = 0, 1
POSE_VIEW_DTYPE = np.dtype([("Rcw", "<f4", 9), ("tcw", "<f4", 3), ("Ow", "<f4", 3), ("_pad", "<f4")])


# ---------------------------------------------------------------- LandMarkMatches
class MapMatches:
    """LandMarkMatches with its two std::maps (Python dicts walked in sorted key order)"""

    def __init__(self):
        self.views_to_landmarks, self.outliers, self.n_matches = {}, {}, 0

    def has(self, i):                                        # hasAssociation(int): the landmark or None
        return self.views_to_landmarks.get(i)

    def view_of(self, lm):                                   # hasAssociation(MapPoint*): the FIRST view in map order, or -1
        for i in sorted(self.views_to_landmarks):
            if self.views_to_landmarks[i] == lm:
                return i
        return -1

    def associate(self, i, lm, replace=True):                # associateLandMark
        if lm is None:
            return -1
        old, idx_old = self.has(i), self.view_of(lm)
        if old is not None or idx_old >= 0:
            if not replace:
                return -1
            self.views_to_landmarks[i] = lm
            self.outliers[i] = False
            if idx_old >= 0 and idx_old != i:
                del self.views_to_landmarks[idx_old]
            return 0
        self.views_to_landmarks[i] = lm
        self.outliers.setdefault(i, False)                   # insert({i, false}): a stale entry stays
        self.n_matches += 1
        return 0

    def remove(self, i):                                     # removeLandMarkAssociation(int)
        if self.has(i) is None:
            return -1
        del self.views_to_landmarks[i]
        self.outliers.pop(i, None)
        self.n_matches -= 1
        return 0

    def clear(self):
        self.views_to_landmarks.clear()
        self.outliers.clear()
        self.n_matches = 0

    def is_outlier(self, i):
        return self.outliers.get(i, False)

    def set_outlier(self, i, flag):
        if i in self.outliers:
            self.outliers[i] = bool(flag)

    def items(self):                                         # a copy, in view order
        return [(i, self.views_to_landmarks[i]) for i in sorted(self.views_to_landmarks)]

    def dense(self, n):
        kp_lm, outl = np.full(n, -1, np.int32), np.zeros(n, np.uint8)
        for i, lm in self.views_to_landmarks.items():
            kp_lm[i] = lm
        for i, o in self.outliers.items():
            outl[i] = 2 if o else 1
        return kp_lm, outl, int(self.n_matches)

    @classmethod
    def from_dense(cls, kp_lm, outl, n_matches):
        m = cls()
        m.views_to_landmarks = {int(i): int(kp_lm[i]) for i in np.nonzero(np.asarray(kp_lm) >= 0)[0]}
        m.outliers = {int(i): bool(outl[i] == 2) for i in np.nonzero(np.asarray(outl))[0]}
        m.n_matches = int(n_matches)
        return m


class DenseMatches:
    """the dense state: kp_lm (-1 = none), kp_outl (0 none / 1 false / 2 true), n_matches"""

    def __init__(self, n):
        self.kp_lm, self.kp_outl, self.n_matches = np.full(n, -1, np.int32), np.zeros(n, np.uint8), 0

    def has(self, i):
        return None if self.kp_lm[i] < 0 else int(self.kp_lm[i])

    def associate(self, i, lm, replace=True):                # hip_detail::assoc_apply
        held = np.nonzero(self.kp_lm == lm)[0]
        j = int(held[0]) if len(held) else -1
        if self.kp_lm[i] < 0 and j < 0:
            self.kp_lm[i] = lm
            if not self.kp_outl[i]:
                self.kp_outl[i] = 1
            self.n_matches += 1
            return 0
        self.kp_lm[i], self.kp_outl[i] = lm, 1
        if j >= 0 and j != i:
            self.kp_lm[j] = -1
        return 0

    def remove(self, i):
        if self.kp_lm[i] < 0:
            return -1
        self.kp_lm[i], self.kp_outl[i] = -1, 0
        self.n_matches -= 1
        return 0

    def clear(self):
        self.kp_lm[:], self.kp_outl[:], self.n_matches = -1, 0, 0

    def is_outlier(self, i):
        return bool(self.kp_outl[i] == 2)

    def set_outlier(self, i, flag):
        if self.kp_outl[i]:
            self.kp_outl[i] = 2 if flag else 1

    def items(self):
        return [(int(i), int(self.kp_lm[i])) for i in np.nonzero(self.kp_lm >= 0)[0]]

    def dense(self, n=None):
        return self.kp_lm.copy(), self.kp_outl.copy(), int(self.n_matches)

    @classmethod
    def from_dense(cls, kp_lm, outl, n_matches):
        m = cls(len(kp_lm))
        m.kp_lm[:], m.kp_outl[:], m.n_matches = kp_lm, outl, int(n_matches)
        return m


def valid_ops(op_view, op_lm, n, L):
    op_view, op_lm = np.asarray(op_view, np.int64), np.asarray(op_lm, np.int64)
    return (op_view >= 0) & (op_view < n) & (op_lm >= 0) & (op_lm < L)


def replay_sequential(matches, op_view, op_lm, n, L):
    """the loop at FeatureMatcher.cc:113-118: the ops in ascending landmark index, one associateLandMark each"""
    ok = np.nonzero(valid_ops(op_view, op_lm, n, L))[0]
    for j in ok[np.argsort(np.asarray(op_lm)[ok], kind="stable")]:
        matches.associate(int(op_view[j]), int(op_lm[j]), True)
    return matches


def replay_closed_form(kp_lm, kp_outl, n_matches, op_view, op_lm, L, minw_strict=False):
    """the kernels' four phases on arrays (k_assoc_writers, k_assoc_holders, k_assoc_erase, k_assoc_final); -> (kp_lm, kp_outl, n_matches).
    minw_strict: the mutation `minw[u] > k` the tests must catch"""
    kp0, outl = np.asarray(kp_lm, np.int64), np.asarray(kp_outl, np.uint8).copy()
    n = len(kp0)
    ok = valid_ops(op_view, op_lm, n, L)
    v, k = np.asarray(op_view, np.int64)[ok], np.asarray(op_lm, np.int64)[ok]
    minw, maxw = np.full(n, NONE, np.int64), np.full(n, -1, np.int64)
    np.minimum.at(minw, v, k)
    np.maximum.at(maxw, v, k)
    jk = np.full(max(L, 1), NONE, np.int64)
    inside = (kp0 >= 0) & (kp0 < L)
    holds = inside & ((minw > kp0) if minw_strict else (minw >= kp0))
    np.minimum.at(jk, kp0[holds], np.nonzero(holds)[0])
    erased = np.zeros(n, bool)
    u = jk[k]
    hit = (u != NONE) & (u != v)
    erased[u[hit]] = True
    out = kp0.copy()
    written = maxw >= 0
    first = np.where(written, minw, 0)
    fresh = written & ((kp0 < 0) | erased) & (jk[np.minimum(first, max(L, 1) - 1)] == NONE)
    out[written] = maxw[written]
    out[~written & erased] = -1
    keep_flag = fresh & (minw == maxw) & (outl != 0)
    outl[written & ~keep_flag] = 1
    return out.astype(np.int32), outl, int(n_matches) + int(fresh.sum())


# ---------------------------------------------------------------- pose
def pose_view(Tcw):
    """Frame::UpdatePoseMatrices: Rcw, tcw copied, Ow = -Rcw^T tcw as one gemm (double accumulation, alpha in double, one rounding)"""
    T = np.asarray(Tcw, f32).reshape(4, 4)
    pv = np.zeros(1, POSE_VIEW_DTYPE)[0]
    pv["Rcw"], pv["tcw"] = T[:3, :3].ravel(), T[:3, 3]
    with np.errstate(all="ignore"):
        pv["Ow"] = [pyref._gemm_row(T[:3, i], T[:3, 3], 0.0, -1.0) for i in range(3)]
    return pv


def pose_view_float(Tcw):
    """the mutation `Ow accumulated in float` the tests must catch"""
    T = np.asarray(Tcw, f32).reshape(4, 4)
    pv = pose_view(T)
    with np.errstate(all="ignore"):
        pv["Ow"] = [-f32(f32(f32(T[0, i] * T[0, 3]) + f32(T[1, i] * T[1, 3])) + f32(T[2, i] * T[2, 3])) for i in range(3)]
    return pv


# ---------------------------------------------------------------- the projection search
class ProjParams:
    def __init__(self, th, score_threshold, second_best_ratio, use_distance, use_stereo, check_rotation, use_prev_matched=1, frac_smaller=0.5, frac_larger=1.5):
        self.th, self.score_threshold, self.second_best_ratio, self.use_distance, self.use_stereo, self.check_rotation = \
            th, score_threshold, second_best_ratio, use_distance, use_stereo, check_rotation
        self.use_prev_matched, self.frac_smaller, self.frac_larger = use_prev_matched, frac_smaller, frac_larger


def _project(fr, pv, P):
    R = pv["Rcw"].reshape(3, 3)
    with np.errstate(all="ignore"):
        Pc = [pyref._gemm_row(R[i], P, pv["tcw"][i]) for i in range(3)]
        u, v, ok = pyref.camera_project(fr, Pc)
        ur = f32(u - f32(f32(fr["mbf"]) * f32(f32(1) / f32(Pc[2])))) if fr["sensor"] == 1 else f32(-1)
    return u, v, ur, ok


def search_by_projection(fr, pv, lms, pp, kp_lm_obs, grid=None):
    """-> (match_idx [L], match_dist [L], n_matches): hs_search_by_projection_posed_device.  fr: fx, fy, cx, cy, mbf, sensor, bounds, kps, desc, uR"""
    kps, desc, uR = fr["kps"], fr["desc"], np.asarray(fr["uR"], f32)
    grid = grid or pyref.AreaGrid(kps, fr["bounds"])
    L = len(lms)
    midx, mdist = np.full(L, -1, np.int32), np.full(L, -1, f32)
    obs = np.asarray(kp_lm_obs)
    for li in range(L):
        lm = lms[li]
        if lm["skip"]:
            continue
        P = lm["pos"].astype(f32)
        u, v, ur, ok = _project(fr, pv, P)
        if not ok:
            continue
        if pp.use_distance:
            d3 = (P - pv["Ow"]).astype(f32)
            dist = pyref._norm(d3)
            if dist < f32(0.8) * lm["min_dist"] or dist > f32(1.2) * lm["max_dist"]:
                continue
        with np.errstate(all="ignore"):
            if lm["assoc_kp"] >= 0:
                size = f32(kps["size"][lm["assoc_kp"]])
            else:
                half = f32(f32(lm["size"]) / f32(2))
                size = f32(_project(fr, pv, [f32(P[0] + half), P[1], P[2]])[0] - _project(fr, pv, [f32(P[0] - half), P[1], P[2]])[0])
            r = f32(f32(f32(pp.th) * size) / f32(31))
            area = grid.features_in_area(u, v, r)
            m = np.ones(len(area), bool)
            if pp.use_prev_matched:
                m &= ~(obs[area] > 0)
            ks = kps["size"][area]
            m &= (ks > f32(pp.frac_smaller) * size) & (ks < f32(pp.frac_larger) * size)
            if pp.use_stereo and fr["sensor"] != 0:
                m &= (np.abs((ur - uR[area]).astype(f32)) < r) & (uR[area] > 0)
        cand = area[m]
        if len(cand) == 0:
            continue
        d = np.unpackbits(desc[cand] ^ lm["desc"][None, :], axis=1).sum(1)
        b = int(np.argmin(d))                                   # first minimum in candidate order
        second = f32(np.sort(d)[1]) if len(d) > 1 else np.finfo(f32).max
        if d[b] <= pp.score_threshold and not (f32(d[b]) > f32(pp.second_best_ratio) * second):
            midx[li], mdist[li] = cand[b], d[b]
    if pp.check_rotation:                                       # RotationConsistencyCriterion on the std::map keyed by keypoint: the last landmark of a keypoint stays
        live = np.nonzero(midx >= 0)[0]
        last = {}
        for i in live:
            last[int(midx[i])] = int(i)
        win = np.array(sorted(last.values()), np.int64)
        midx[np.setdiff1d(live, win)] = -1
        if len(win):
            bins, _ = ref_bow.rotation_bins(kps["angle"][midx[win]], lms["prev_angle"][win])      # rot = prev_angle - angle
            keep_bins = [i for i in ref_bow.three_maxima(np.bincount(bins, minlength=30)) if i >= 0]
            midx[win[~np.isin(bins, keep_bins)]] = -1
    # the distance of a dropped match stays, as the kernel leaves it
    return midx, mdist, int((midx >= 0).sum())


# ---------------------------------------------------------------- the two strategies
class TrackParams:
    def __init__(self, th_motion=15.0, th_motion_wide=30.0, n_min_matches=20, th_local=3.0, nnratio_motion=0.9, nnratio_local=0.8, th_high=100.0, sigma_ref=1.0,
                 n_max_local_keyframes=80, n_neighbor_keyframes=10):
        self.th_motion, self.th_motion_wide, self.n_min_matches, self.th_local = th_motion, th_motion_wide, n_min_matches, th_local
        self.nnratio_motion, self.nnratio_local, self.th_high, self.sigma_ref = nnratio_motion, nnratio_local, th_high, sigma_ref
        self.n_max_local_keyframes, self.n_neighbor_keyframes = n_max_local_keyframes, n_neighbor_keyframes


def gather_last(lms, last_kp_lm, last_kps):
    """record j = the landmark of last-frame keypoint j: skip = 1 without one, assoc_kp = -1, prev_angle = the keypoint's angle"""
    L = len(lms)
    out = np.zeros(len(last_kp_lm), lms.dtype)
    ok = (np.asarray(last_kp_lm) >= 0) & (np.asarray(last_kp_lm) < L)
    out[ok] = lms[np.asarray(last_kp_lm)[ok]]
    out["assoc_kp"] = -1
    out["skip"] = np.where(ok, 0, 1)
    out["prev_angle"] = np.where(ok, last_kps["angle"], 0)
    return out


def lm_obs_of(matches, n, lm_nobs):
    obs = np.full(n, -1, np.int32)
    for i, lm in matches.items():
        obs[i] = lm_nobs[lm]
    return obs


def optimize(fr, Tcw, matches, lms, tp, run=True):
    """Optimizer::PoseOptimization on the frame: the edges in keypoint order, the result, and setOutlier on every edge when it ran"""
    n = len(fr["kps"])
    kp_lm, _, _ = matches.dense(n)
    edges, n_edges = RP.gather_edges(fr["kps"], fr["uR"], kp_lm, lms["pos"], 31.0, tp.sigma_ref)
    cam = np.array([fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["mbf"]], f32)
    res = RP.pose_optimization_fast(Tcw, cam, edges if run else edges[:0])
    if res["status"] != RP.STATUS_TOO_FEW:
        for k in range(len(edges)):
            matches.set_outlier(int(edges["kp"][k]), bool(res["outlier"][k]))
    return edges, n_edges, res, cam


def discard(matches, mode, sensor, lm_nobs):
    """TrackMotionModel.cpp:62-79 / TrackLocalMap.cpp:25-38 -> the count"""
    count = 0
    for i, lm in matches.items():
        if matches.is_outlier(i):
            if mode == MOTION or sensor == 1:
                matches.remove(i)
                matches.set_outlier(i, False)                   # "legacy": the entry is gone, nothing happens
        elif lm_nobs[lm] > 0:
            count += 1
    return count


def track_motion_model(fr, Tcw_pred, last_kps, last_kp_lm, lms, lm_nobs, tp, matches, pv=None, grid=None):
    """-> dict of every stage's result; `matches` (MapMatches or DenseMatches) is updated in place"""
    n, L = len(fr["kps"]), len(lms)
    out = dict(pose_view=pv if pv is not None else pose_view(Tcw_pred))
    out["last_lms"] = gather_last(lms, last_kp_lm, last_kps)
    matches.clear()
    obs = np.full(n, -1, np.int32)
    grid = grid or pyref.AreaGrid(fr["kps"], fr["bounds"])
    for name, th in (("narrow", tp.th_motion), ("wide", tp.th_motion_wide)):
        pp = ProjParams(th, tp.th_high, tp.nnratio_motion, 0, 1, 1)
        out[name + "_idx"], out[name + "_dist"], out[name + "_n"] = search_by_projection(fr, out["pose_view"], out["last_lms"], pp, obs, grid)
    wide = out["narrow_n"] < tp.n_min_matches
    chosen = out["wide_idx"] if wide else out["narrow_idx"]
    failed = (out["wide_n"] if wide else out["narrow_n"]) < tp.n_min_matches
    out.update(op_view=chosen.copy(), used_wide=int(wide), status=TRACK_MOTION_FAILED if failed else TRACK_OK)
    replay_sequential(matches, chosen, last_kp_lm, n, L)
    out["after_associate"] = matches.dense(n)
    out["edges"], out["n_edges"], out["pose"], out["cam"] = optimize(fr, Tcw_pred, matches, lms, tp, run=not failed)
    out["n_edges_run"] = 0 if failed else out["n_edges"]
    out["n_matches_map"] = 0 if failed else discard(matches, MOTION, fr["sensor"], lm_nobs)
    out["state"] = matches.dense(n)
    return out


def track_local_map(fr, Tcw_in, T, lms, neigh, parent, cap, tp, matches, pv=None, grid=None):
    n, L = len(fr["kps"]), len(lms)
    out = dict(pose_view=pv if pv is not None else pose_view(Tcw_in))
    for i, lm in matches.items():                               # SearchLocalPoints :56-67
        if T["lm_bad"][lm]:
            matches.remove(i)
    obs = lm_obs_of(matches, n, T["lm_nobs"])
    kp_lm, _, _ = matches.dense(n)
    held = kp_lm[kp_lm >= 0]                                    # the kernels skip a null entry
    w = RK.votes_fast(T, np.array([0, len(held)], np.int64), held, None, 1, 1, 0)
    loc, n_local = RL.local_keyframes_fast(w["weights"][0], T["kf_bad"], neigh, parent, tp.n_max_local_keyframes, tp.n_neighbor_keyframes)
    pts = RL.local_points_fast(T, loc, kp_lm, cap)
    out.update(kp_lm_obs=obs, weights=w["weights"][0], max_slot=w["max_slot"][0], max_count=w["max_count"][0], local=loc, n_local=n_local,
               frame_remove=pts["frame_remove"], sel=pts["sel"], n_sel=pts["n_sel"])
    out["lms"] = RL.gather(lms, pts["sel"], pts["n_sel"], cap)
    pp = ProjParams(tp.th_local, tp.th_high, tp.nnratio_local, 1, 1, 0)
    out["match_idx"], out["match_dist"], out["n_matches"] = search_by_projection(fr, out["pose_view"], out["lms"], pp, obs, grid)
    replay_sequential(matches, out["match_idx"], pts["sel"], n, L)
    out["after_associate"] = matches.dense(n)
    out["edges"], out["n_edges"], out["pose"], out["cam"] = optimize(fr, Tcw_in, matches, lms, tp)
    out["n_inliers"] = discard(matches, LOCAL, fr["sensor"], T["lm_nobs"])
    out["state"] = matches.dense(n)
    return out


def track_frame(c, matches, motion=None):
    """both stages on a case of track_cases; `motion`: a stage-1 result to continue from (its state is loaded into `matches`)"""
    fr, tp = c["frame"], c["tp"]
    grid = pyref.AreaGrid(fr["kps"], fr["bounds"])
    if motion is None:
        motion = track_motion_model(fr, c["Tcw_pred"], c["last_kps"], c["last_kp_lm"], c["lms"], c["T"]["lm_nobs"], tp, matches, grid=grid)
    local = track_local_map(fr, motion["pose"]["Tcw"], c["T"], c["lms"], c["neigh"], c["parent"], c["cap"], tp, matches, grid=grid)
    return motion, local
