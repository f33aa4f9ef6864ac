"""Cases for the key-frame decision and stereo landmark creation (tests/ref_keyframe.py; tests/test_keyframe_ref.py on the CPU, tests/test_gpu_keyframe.py
on the device).  Every generator is a pure function of its arguments.

  make(...)        a case from explicit arrays (the exhaustive space and the directed cases)
  seeded(seed, n)  a random case of n views
  DIRECTED         name -> (case, witness): the witness takes the literal result and says whether the case's edge occurred"""
import numpy as np

import ref_keyframe as RKF

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])
f32 = np.float32
TH = 40.0
GOOD_TRACK = dict(status=0, n_matches_map=50, n_inliers=120)            # ok, and tracking_weak with the default target 200 - 50
# an inserting set of parameters for small cases: the interval is exceeded, so `definite_insert`
INSERT = dict(frame_id=100, last_keyframe_id=10, max_KF_interval=30, th_depth=TH)


def pose(seed=3):
    rng = np.random.default_rng(seed)
    T = np.eye(4, dtype=f32)
    T[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    T[:3, 3] = rng.normal(0, 3, 3)
    return T


def table(L, n_kf, lm_nobs=None, lm_bad=None, kf_bad=None, obs=None):
    """landmark l is observed by key frames obs[l] (default: l % n_kf and (l + 1) % n_kf, ascending)"""
    obs = obs if obs is not None else [sorted({l % n_kf, (l + 1) % n_kf}) for l in range(L)] if n_kf else [[] for _ in range(L)]
    off = np.zeros(L + 1, np.int64)
    np.cumsum([len(o) for o in obs], out=off[1:])
    kf = np.array([s for o in obs for s in o], np.int32)
    return dict(lm_obs_offsets=off, lm_obs_kf=kf, lm_obs_octave=np.zeros(len(kf), np.int32),
                lm_bad=np.zeros(L, np.uint8) if lm_bad is None else np.asarray(lm_bad, np.uint8),
                lm_nobs=np.array([len(o) for o in obs], np.int32) if lm_nobs is None else np.asarray(lm_nobs, np.int32),
                kf_bad=np.zeros(n_kf, np.uint8) if kf_bad is None else np.asarray(kf_bad, np.uint8), kf_id=np.arange(n_kf, dtype=np.int64) + 100)


def keyframes(lists):
    """K from one list of landmark indices per key frame"""
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    return dict(n_kf=len(lists), kf_off=off, kp_lm=np.array([x for l in lists for x in l], np.int32))


def frame(n, sensor=1, seed=11):
    rng = np.random.default_rng(seed)
    kps = np.zeros(n, KP_DTYPE)
    kps["x"], kps["y"] = rng.uniform(0, 1240, n).astype(f32), rng.uniform(0, 370, n).astype(f32)
    kps["size"] = (31 * 1.2 ** rng.integers(0, 8, n)).astype(f32)
    return dict(fx=718.856, fy=716.5, cx=607.19, cy=185.2, mbf=386.1, sensor=sensor, bounds=(0.0, 1241.0, 0.0, 376.0), kps=kps,
                desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), uR=np.full(n, -1, f32))


def make(depth, kp_lm, kp_outl, L=3, n_kf=3, lm_nobs=None, lm_bad=None, kf_bad=None, obs=None, K=None, n_matches=None, sensor=1, track=None, ref_slot=0, new_cap=None,
         Tcw=None, **prm):
    depth, kp_lm, kp_outl = np.asarray(depth, f32), np.asarray(kp_lm, np.int32), np.asarray(kp_outl, np.uint8)
    n = len(depth)
    assert len(kp_lm) == n and len(kp_outl) == n
    T = table(L, n_kf, lm_nobs, lm_bad, kf_bad, obs)
    K = K if K is not None else keyframes([[(s + j) % L if L else -1 for j in range(2)] for s in range(n_kf)])
    return dict(state=(kp_lm, kp_outl, int((kp_lm >= 0).sum()) if n_matches is None else n_matches), T=T, K=K, depth=depth, frame=frame(n, sensor),
                Tcw=pose() if Tcw is None else Tcw, track=dict(track or GOOD_TRACK), prm=RKF.params(**dict(INSERT, **prm)), ref_slot=ref_slot,
                new_cap=n if new_cap is None else new_cap)


def seeded(seed, n, L=None, n_kf=5, ref_kp=None, sensor=1, **prm):
    """a random case: depths from a coarse grid (ties), a fifth without depth, held / empty views with every flag, bad and unobserved landmarks"""
    rng = np.random.default_rng(seed)
    L = L or max(3, n // 2)
    depth = rng.integers(1, 81, n).astype(f32)
    no = rng.random(n) < 0.2
    depth[no] = rng.choice(np.array([-1.0, 0.0, np.nan], f32), int(no.sum()))
    kp_lm = np.where(rng.random(n) < 0.5, rng.integers(0, L, n), -1).astype(np.int32)
    kp_outl = np.where(kp_lm >= 0, rng.choice(np.array([0, 1, 1, 1, 2], np.uint8), n), rng.choice(np.array([0, 0, 1, 2], np.uint8), n)).astype(np.uint8)
    obs = [sorted(set(rng.integers(0, n_kf, rng.integers(0, 4)).tolist())) for _ in range(L)]
    lm_nobs = np.array([len(o) * rng.integers(1, 3) for o in obs], np.int32)
    lm_nobs[rng.random(L) < 0.1] = 0
    sizes = [int(rng.integers(0, 2 * n + 2)) for _ in range(n_kf)]
    if ref_kp is not None:
        sizes = [ref_kp] * n_kf
    K = keyframes([rng.integers(-1, L, s).tolist() for s in sizes])
    p = dict(n_min_points=int(rng.integers(0, n + 2)), th_depth=float(rng.integers(10, 70)), min_N_tracked_close=int(rng.integers(0, n + 1)),
             thresh_N_nontracked_close=int(rng.integers(0, n // 2 + 1)))
    p.update(prm)
    return make(depth, kp_lm, kp_outl, L=L, n_kf=n_kf, lm_nobs=lm_nobs, lm_bad=(rng.random(L) < 0.1), kf_bad=(rng.random(n_kf) < 0.2), obs=obs, K=K,
                n_matches=int((kp_lm >= 0).sum()) + int(rng.integers(0, 3)), sensor=sensor, ref_slot=int(rng.integers(-1, n_kf)), Tcw=pose(seed), **p)


GPU_SIZES = [1, 63, 64, 65, 1025, 2049]


def gpu_seeded(n, seed):
    """the 8 seeded cases per size of tests/test_gpu_keyframe.py: reference key frames of 0, 1 and 1025 keypoints, every fourth not inserting, new_cap
    below, at and above n_new"""
    quiet = dict(frame_id=12, N_tracked_target=100, N_tracked_variance=10, min_N_tracked_close=0) if seed % 4 == 3 else {}      # nothing asks for a key frame
    c = seeded(7700 + 100 * seed + n, n, ref_kp=(0, 1, 1025)[seed % 3], n_kf=3, **quiet)
    n_new = RKF.dense(c)["result"]["n_new"]
    c["new_cap"] = (max(n_new - 1, 0), n_new, n_new + 3)[(seed // 3) % 3]
    return c


# ---------------------------------------------------------------- directed cases
E, H = -1, 0                                                     # an empty view / a view that holds landmark 0 (observed, good)


def _far_list(n_points, extra):
    """n_points close views then `extra` far ones, all empty: the list has n_min_points + extra entries"""
    d = [10.0 + i for i in range(n_points)] + [TH + 1 + i for i in range(extra)]
    return make(d, [E] * len(d), [0] * len(d), n_min_points=n_points)


def _decision(**prm):
    """a frame that tracks well (n_inliers above every target), no interval exceeded, mapping idle: nothing asks for a key frame until `prm` does"""
    base = dict(frame_id=12, last_keyframe_id=10, max_KF_interval=30, min_KF_interval=0, N_tracked_target=100, N_tracked_variance=10, min_N_tracked_close=0)
    return make([10.0, 20.0, 50.0], [H, E, E], [1, 0, 0], **dict(base, **prm))


DIRECTED = {
    # a list of exactly n_min_points, +1 and +2 entries with far points: the break needs nPoints > n_min_points AND a far point
    "list_is_n_min_points": (_far_list(3, 0), lambda r: r["result"]["n_processed"] == 3 == r["result"]["n_candidates"]),
    "list_is_n_min_points_plus_1": (_far_list(3, 1), lambda r: r["result"]["n_processed"] == 4 == r["result"]["n_candidates"]),
    "list_is_n_min_points_plus_2": (_far_list(3, 2), lambda r: r["result"]["n_processed"] == 4 and r["result"]["n_candidates"] == 5),
    # the far points start before n_min_points: the walk goes on to n_min_points
    "far_before_n_min_points": (make([10.0, 50.0, 60.0, 70.0, 80.0], [E] * 5, [0] * 5, n_min_points=3), lambda r: r["result"]["n_processed"] == 4),
    "n_min_points_zero": (make([10.0, 50.0, 60.0], [E] * 3, [0] * 3, n_min_points=0), lambda r: r["result"]["n_processed"] == 2),
    # depth == th_depth is not far (`>`): the walk runs to the view behind it
    "depth_equals_th_depth": (make([TH, 10.0, 50.0, 60.0], [E] * 4, [0] * 4, n_min_points=0),
                              lambda r: r["result"]["n_processed"] == 3 and r["new_view"].tolist() == [1, 0, 2]),
    # equal depths: ascending index, whatever the array order suggests
    "equal_depths": (make([30.0, 20.0, 20.0, 20.0, 10.0], [E] * 5, [0] * 5), lambda r: r["new_view"].tolist() == [4, 1, 2, 3, 0]),
    "equal_depths_cut": (make([50.0, 50.0, 50.0, 10.0], [E] * 4, [0] * 4, n_min_points=2), lambda r: r["new_view"].tolist() == [3, 0, 1]),
    "inf_and_nan_depth": (make([np.inf, np.nan, 10.0, -np.inf], [E] * 4, [0] * 4), lambda r: r["new_view"].tolist() == [2, 0] and r["result"]["n_candidates"] == 2),
    "nan_th_depth": (make([10.0, 50.0, 60.0, 70.0], [E] * 4, [0] * 4, n_min_points=0, th_depth=float("nan")),
                     lambda r: r["result"]["n_processed"] == 4 and r["result"]["n_tracked_close"] + r["result"]["n_nontracked_close"] == 0),
    "empty_list": (make([0.0, -1.0, np.nan], [E, H, E], [0, 1, 2]), lambda r: r["result"]["insert"] == 1 and r["result"]["n_candidates"] == 0 == r["result"]["n_new"]),
    # a held view whose landmark nobody observes: removed and re-created in stage 5 when stage 3 is not run; in the composite stage 3 removes it first
    "held_unobserved": (make([10.0, 20.0], [1, H], [2, 1], lm_nobs=[2, 0, 2]),
                        lambda r: r["kp_lm"].tolist() == [3, 0] and r["kp_outl"].tolist() == [1, 1] and r["n_matches"] == 2),
    "empty_stale_flag_2": (make([10.0, 20.0], [E, E], [2, 1]), lambda r: r["kp_lm"].tolist() == [-1, 4] and r["result"]["n_new"] == 2),
    "landmark_on_two_views": (make([10.0, 20.0, 30.0], [1, 1, 0], [1, 1, 1], obs=[[0], [1], [2]], kf_bad=[0, 0, 0]),
                              lambda r: r["result"]["ref_slot"] == 1),
    "vote_without_winner": (make([10.0, 20.0], [E, E], [0, 0], ref_slot=2), lambda r: r["result"]["ref_slot"] == 2),
    "vote_all_bad_landmarks": (make([10.0, 20.0], [0, 1], [1, 1], lm_bad=[1, 1, 0], ref_slot=1), lambda r: r["result"]["ref_slot"] == 1 and r["n_matches"] == 2),
    "bad_winner": (make([10.0, 20.0, 30.0], [0, 0, 1], [1, 1, 1], obs=[[0], [2], [1]], kf_bad=[1, 0, 0]), lambda r: r["result"]["ref_slot"] == 2),
    "equal_votes_lowest_slot": (make([10.0, 20.0], [0, 1], [1, 1], obs=[[2], [1], [0]]), lambda r: r["result"]["ref_slot"] == 1),
    "not_ok_status": (make([10.0], [E], [0], track=dict(status=1, n_matches_map=50, n_inliers=120)), lambda r: r["result"]["ok"] == 0 == r["result"]["insert"]),
    "not_ok_init": (make([10.0], [E], [0], track=dict(status=0, n_matches_map=10, n_inliers=120)), lambda r: r["result"]["ok"] == 0),
    "not_ok_refine": (make([10.0], [E], [0], track=dict(status=0, n_matches_map=50, n_inliers=30)), lambda r: r["result"]["ok"] == 0),
    "not_ok_force_loss": (make([10.0, 20.0], [E, H], [0, 2], force_loss=1), lambda r: r["result"]["ok"] == 0 and r["kp_lm"].tolist() == [-1, 0]),
    "ok_just_above": (make([10.0], [E], [0], track=dict(status=0, n_matches_map=11, n_inliers=31)), lambda r: r["result"]["ok"] == 1),
    "override_0": (make([10.0], [E], [0], ok_override=0), lambda r: r["result"]["ok"] == 0),
    # each term of the decision flipped alone
    "decision_none": (_decision(), lambda r: r["result"]["insert"] == 0),
    "decision_force": (_decision(force=1), lambda r: r["result"]["insert"] == 1),
    "decision_max_interval": (_decision(frame_id=40), lambda r: r["result"]["insert"] == 1),
    "decision_max_interval_below": (_decision(frame_id=39), lambda r: r["result"]["insert"] == 0),
    "decision_dire": (_decision(N_tracked_target=141), lambda r: r["result"]["insert"] == 1),
    "decision_weak": (_decision(N_tracked_target=131), lambda r: r["result"]["insert"] == 1),
    "decision_weak_min_interval": (_decision(N_tracked_target=131, min_KF_interval=3), lambda r: r["result"]["insert"] == 0),
    "decision_weak_busy_short_queue": (_decision(N_tracked_target=131, mapping_idle=0, mapping_queue_length=0), lambda r: r["result"]["insert"] == 0),
    "decision_dire_busy_short_queue": (_decision(N_tracked_target=141, mapping_idle=0, mapping_queue_length=2), lambda r: r["result"]["insert"] == 1),
    "decision_dire_busy_long_queue": (_decision(N_tracked_target=141, mapping_idle=0, mapping_queue_length=3), lambda r: r["result"]["insert"] == 0),
    "decision_lack_close": (_decision(min_N_tracked_close=2, thresh_N_nontracked_close=0),
                            lambda r: r["result"]["insert"] == 1 and (r["result"]["n_tracked_close"], r["result"]["n_nontracked_close"]) == (1, 1)),
    "decision_lack_close_threshold": (_decision(min_N_tracked_close=2, thresh_N_nontracked_close=1), lambda r: r["result"]["insert"] == 0),
    "decision_enough_close": (_decision(min_N_tracked_close=1, thresh_N_nontracked_close=0), lambda r: r["result"]["insert"] == 0),
    "decision_mapping_stopped": (_decision(force=0, frame_id=40, mapping_stopped=1), lambda r: r["result"]["insert"] == 0),
    "decision_mapping_stopped_forced": (_decision(force=1, mapping_stopped=1), lambda r: r["result"]["insert"] == 1),
    "decision_interval_wraps": (_decision(frame_id=5, last_keyframe_id=0xFFFFFFF0, max_KF_interval=30, N_tracked_target=0, min_KF_interval=100),
                                lambda r: r["result"]["insert"] == 0),
    "decision_interval_wraps_exceeded": (_decision(frame_id=14, last_keyframe_id=0xFFFFFFF0, max_KF_interval=30), lambda r: r["result"]["insert"] == 1),
    "decision_frame_id_64_bits": (_decision(frame_id=(1 << 32) + 1, last_keyframe_id=10), lambda r: r["result"]["insert"] == 1),
    # an outlier view is not tracked-close
    "outlier_not_tracked_close": (make([10.0, 20.0, 30.0], [0, 1, E], [2, 1, 0], min_N_tracked_close=0),
                                  lambda r: (r["result"]["n_tracked_close"], r["result"]["n_nontracked_close"]) == (1, 2)),
    "sensor_mono": (make([10.0, 20.0], [E, H], [0, 2], sensor=0),
                    lambda r: r["result"]["insert"] == 1 and r["result"]["n_candidates"] == 0 and r["result"]["n_nontracked_close"] == 0 and r["kp_lm"].tolist() == [-1, -1]),
    "ref_slot_outside": (make([10.0], [E], [0], ref_slot=-1), lambda r: r["result"]["ref_slot"] == -1 and r["result"]["n_ref_matches"] == 0),
    "ref_slot_past_the_end": (make([10.0], [E], [0], ref_slot=7), lambda r: r["result"]["ref_slot"] == 7 and r["result"]["n_ref_matches"] == 0),
    "ref_matches_min_obs": (make([10.0], [H], [1], L=4, lm_nobs=[3, 2, 3, 1], lm_bad=[0, 0, 1, 0], K=keyframes([[0, 1, 2, 3, -1, 0]] * 3), n_kfs_in_map=3),
                            lambda r: r["result"]["n_ref_matches"] == 2),
    "ref_matches_few_key_frames": (make([10.0], [H], [1], L=4, lm_nobs=[3, 2, 3, 1], lm_bad=[0, 0, 1, 0], K=keyframes([[0, 1, 2, 3, -1, 0]] * 3), n_kfs_in_map=2),
                                   lambda r: r["result"]["n_ref_matches"] == 3),
    # a state that still holds provisional indices (>= L) from the last insert: no table is read through them; the outlier among them is removed
    # (a frame that does not insert: a new point would be numbered L + 0 again, so the caller appends before the next insert)
    "provisional_in_input": (make([10.0, 20.0, 30.0, 35.0], [3, 4, H, E], [1, 2, 1, 0], frame_id=12, N_tracked_target=100, N_tracked_variance=10,
                                  min_N_tracked_close=0),
                             lambda r: r["kp_lm"].tolist() == [3, -1, 0, -1] and r["kp_lm_obs"].tolist() == [-1, -1, 2, -1] and r["n_matches"] == 2
                             and (r["result"]["n_tracked_close"], r["result"]["n_nontracked_close"]) == (2, 2)),
    "truncated_records": (make([10.0, 20.0, 30.0, 35.0], [E] * 4, [0] * 4, new_cap=2), lambda r: r["result"]["n_new"] == 4 and len(r["entries"]) == 2),
    "final_outlier_removed": (make([10.0, 20.0], [0, 1], [2, 1], min_KF_interval=0, frame_id=12, N_tracked_target=100, N_tracked_variance=10),
                              lambda r: r["kp_lm"].tolist() == [-1, 1] and r["n_matches"] == 1 and r["result"]["n_valid"] == 1),
}
