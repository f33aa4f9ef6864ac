"""Cases for the resident tracking chain (tests/test_track_ref.py on the CPU, tests/test_gpu_track.py on the device): a poseopt_cases scene taken
apart into a current frame (keypoints, descriptors, uR), a map (hs_landmark records, an observation table of a few key frames) and a last frame that
holds some of the map's landmarks, plus the replay states of the association tests.  Every generator is a pure function of its named seed.

A tracking case QUALIFIES like a pose-optimisation case (poseopt_cases.qualify): both optimiser problems of the reference chain keep every
classification MARGIN away from its threshold under the seeded summation orders, so the device's fp64 sums cannot flip an outlier flag."""
import functools

import numpy as np

import poseopt_cases as PC
import ref_track as R

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])
LM_DTYPE = np.dtype([("pos", "<f4", 3), ("size", "<f4"), ("min_dist", "<f4"), ("max_dist", "<f4"), ("normal", "<f4", 3),
                     ("assoc_kp", "<i4"), ("prev_angle", "<f4"), ("skip", "<i4"), ("desc", "u1", 32)])
N_KF = 6
RANDOM_BASE, N_RANDOM = 424243, 12


def build(seed, n=300, n_last=200, extra=100, sensor=1, outliers=0.15, edit=None, tp=None, n_kf=N_KF, max_obs=3):
    """-> the case dict: frame (fx .. uR), Tcw_pred, last_kps, last_kp_lm, lms, T, neigh, parent, cap, tp.  `edit(case, rng, info)` makes a directed case"""
    kind = "stereo" if sensor == 1 else "mono"
    T0, cam, e, d = PC._scene(seed, n, kind, outliers)
    rng = np.random.default_rng(seed + 7)
    fx, fy, cx, cy, bf = (float(c) for c in cam)
    kps = np.zeros(n, KP_DTYPE)
    kps["x"], kps["y"], kps["size"] = e["u"], e["v"], d["size"]
    kps["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    kps["octave"] = np.round(np.log(d["size"] / 31.0) / np.log(1.2)).astype(np.int32)
    uR = e["ur"].astype(np.float32)
    L = n + extra
    slot = rng.permutation(L)[:n].astype(np.int32)                          # map index of scene point i
    lms = np.zeros(L, LM_DTYPE)
    lms["pos"] = rng.normal(0, 40, (L, 3)).astype(np.float32)              # the extra landmarks lie anywhere
    lms["pos"][slot] = e["Xw"]
    Tt = d["Ttrue"].astype(np.float64)
    pc = lms["pos"].astype(np.float64) @ Tt[:3, :3].T + Tt[:3, 3]
    dist = np.linalg.norm(pc, axis=1)
    size_px = np.full(L, 31.0)
    size_px[slot] = d["size"]
    lms["size"] = (size_px * np.abs(pc[:, 2]) / fx * rng.uniform(0.9, 1.1, L)).astype(np.float32)
    lms["min_dist"], lms["max_dist"] = (dist * 0.5).astype(np.float32), (dist * 2.0).astype(np.float32)
    lms["normal"] = (pc / dist[:, None]).astype(np.float32)
    lms["assoc_kp"] = -1
    lms["desc"] = rng.integers(0, 256, (L, 32), dtype=np.uint8)
    desc = lms["desc"][slot].copy()
    for i in range(n):                                                      # the keypoint sees its landmark's descriptor with a few bits flipped
        for b in rng.integers(0, 256, rng.integers(0, 12)):
            desc[i, b >> 3] ^= 1 << (b & 7)
    frame = dict(fx=fx, fy=fy, cx=cx, cy=cy, mbf=bf, sensor=sensor, bounds=(0.0, float(PC.WIDTH), 0.0, float(PC.HEIGHT)), kps=kps, desc=desc, uR=uR)
    # the last frame saw n_last keypoints; most hold the landmark of a scene point, in a shuffled order; the angle moved a little, for a tenth anywhere
    seen = rng.permutation(n)[:n_last]
    last_kp_lm = slot[seen].astype(np.int32)
    last_kp_lm[rng.random(n_last) < 0.1] = -1
    last_kps = np.zeros(n_last, KP_DTYPE)
    last_kps["angle"] = ((kps["angle"][seen] + rng.normal(0, 2, n_last) + (rng.random(n_last) < 0.1) * rng.uniform(0, 360, n_last)) % 360).astype(np.float32)
    # the map: every landmark is observed by a run of 1 .. max_obs of the n_kf key frames
    cnt = rng.integers(1, max_obs + 1, L)
    off = np.zeros(L + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    owner = np.repeat(np.arange(L), cnt)
    start = np.minimum(rng.integers(0, n_kf, L), n_kf - cnt)
    T = dict(lm_obs_offsets=off, lm_obs_kf=(start[owner] + np.arange(int(off[-1])) - off[owner]).astype(np.int32),
             lm_obs_octave=rng.integers(0, 8, int(off[-1])).astype(np.int32), lm_bad=np.zeros(L, np.uint8), lm_nobs=cnt.astype(np.int32),
             kf_bad=np.zeros(n_kf, np.uint8), kf_id=(np.arange(n_kf) + 100).astype(np.int64))
    neigh = np.full((n_kf, 10), -1, np.int32)
    for s in range(n_kf):
        others = rng.permutation(np.setdiff1d(np.arange(n_kf), [s]))[:3]
        neigh[s, :len(others)] = others
    parent = np.full(n_kf, -1, np.int32)
    c = dict(seed=seed, frame=frame, Tcw_pred=T0.astype(np.float32), last_kps=last_kps, last_kp_lm=last_kp_lm, lms=lms, T=T, neigh=neigh, parent=parent, cap=L,
             tp=tp or R.TrackParams(), slot=slot, seen=seen, bad_points=d["bad"])
    if edit:
        edit(c, rng)
    return c


def reference(c):
    """the reference chain on the dense model -> (motion, local)"""
    return R.track_frame(c, R.DenseMatches(len(c["frame"]["kps"])))


def qualifies(c, ref=None):
    """both optimiser problems of the chain under poseopt_cases.qualify (margins under the seeded summation orders); a problem that does not run
    (fewer than 3 edges, or a failed motion stage) has nothing to qualify"""
    motion, local = ref or reference(c)
    for stage, T_in, run in ((motion, c["Tcw_pred"], motion["status"] == R.TRACK_OK), (local, motion["pose"]["Tcw"], True)):
        if run and len(stage["edges"]) >= 3 and PC.qualify(T_in, stage["cam"], stage["edges"]) is None:
            return False
    return True


# ---- directed cases: (builder arguments, what must hold in the reference's result)
def _few_matches(keep):
    def edit(c, rng):                                                       # only `keep` last-frame keypoints hold a landmark
        held = np.nonzero(c["last_kp_lm"] >= 0)[0]
        c["last_kp_lm"][held[keep:]] = -1
    return edit


def _shift_prediction(c, rng):                                              # a prediction so far off that only the wide window finds enough
    c["Tcw_pred"] = c["Tcw_pred"].copy()
    c["Tcw_pred"][0, 3] += np.float32(0.35)


def _no_observations(c, rng):                                               # Observations() == 0 on landmarks the last frame holds
    held = c["last_kp_lm"][c["last_kp_lm"] >= 0]
    c["T"]["lm_nobs"][held[::5]] = 0


def _bad_landmarks(c, rng):                                                 # landmarks the motion stage puts on the frame are bad by stage 2
    held = c["last_kp_lm"][c["last_kp_lm"] >= 0]
    c["T"]["lm_bad"][held[::7]] = 1


def _empty_last(c, rng):
    c["last_kp_lm"][:] = -1


def _threshold_is_the_count(c, rng):                                        # N_min_matches == the narrow search's count: `<` keeps the narrow window
    m = R.track_motion_model(c["frame"], c["Tcw_pred"], c["last_kps"], c["last_kp_lm"], c["lms"], c["T"]["lm_nobs"], c["tp"], R.DenseMatches(len(c["frame"]["kps"])))
    c["tp"] = R.TrackParams(n_min_matches=m["narrow_n"])


DIRECTED = {
    "narrow": (dict(), lambda m, l: m["status"] == 0 and not m["used_wide"]),
    "threshold_exact": (dict(edit=_threshold_is_the_count), lambda m, l: m["status"] == 0 and not m["used_wide"] and m["narrow_n"] < m["wide_n"]),
    "wide": (dict(edit=_shift_prediction, tp=R.TrackParams(n_min_matches=60)), lambda m, l: m["status"] == 0 and m["used_wide"] and m["narrow_n"] < 60 <= m["wide_n"]),
    "both_fail": (dict(edit=_few_matches(12)), lambda m, l: m["status"] == 1 and m["used_wide"] and m["pose"]["status"] == 1 and m["after_associate"][2] > 0),
    "outlier_removed": (dict(outliers=0.3), lambda m, l: m["pose"]["outlier"].sum() > 0 and m["state"][2] < m["after_associate"][2]),
    "zero_observations": (dict(edit=_no_observations), lambda m, l: m["n_matches_map"] < m["pose"]["n_good"]),
    "bad_landmark": (dict(edit=_bad_landmarks), lambda m, l: (l["kp_lm_obs"] >= 0).sum() < (m["state"][0] >= 0).sum()),
    "mono_keeps_outliers": (dict(sensor=0, outliers=0.3, tp=R.TrackParams(th_local=15.0)), lambda m, l: l["pose"]["outlier"].sum() > 0 and (l["state"][1] == 2).any()),
    "stereo_removes_outliers": (dict(sensor=1, outliers=0.3, tp=R.TrackParams(th_local=15.0)), lambda m, l: l["pose"]["outlier"].sum() > 0 and not (l["state"][1] == 2).any()),
    "too_few_edges": (dict(edit=_few_matches(2), tp=R.TrackParams(n_min_matches=1)), lambda m, l: m["status"] == 0 and m["pose"]["status"] == 1 and m["n_edges"] < 3),
    "empty_last": (dict(edit=_empty_last), lambda m, l: m["status"] == 1 and m["wide_n"] == 0 and m["n_edges"] == 0),
    "chunk_1025": (dict(n=1025, n_last=600, extra=200), lambda m, l: m["status"] == 0 and l["n_edges"] > 600),
}
DIRECTED_BASE = {name: 90001 + 1000 * k for k, name in enumerate(DIRECTED)}


@functools.lru_cache(maxsize=None)
def directed(name):
    """-> (case, (motion, local)) of the first seed whose reference result has the directed property and qualifies"""
    args, holds = DIRECTED[name]
    for seed in range(DIRECTED_BASE[name], DIRECTED_BASE[name] + 40):
        c = build(seed, **args)
        ref = reference(c)
        if holds(*ref) and qualifies(c, ref):
            return c, ref
    raise AssertionError("no qualifying seed for " + name)


@functools.lru_cache(maxsize=None)
def random_cases():
    """-> (cases [(case, reference)], seeds drawn): seeds from RANDOM_BASE on until N_RANDOM qualify"""
    out, drawn = [], 0
    while len(out) < N_RANDOM:
        c = build(RANDOM_BASE + drawn, sensor=1 if drawn % 3 else 0)
        drawn += 1
        ref = reference(c)
        if qualifies(c, ref):
            out.append((c, ref))
        assert drawn <= 2 * N_RANDOM, "more than half of the drawn seeds rejected"
    return out, drawn


# ---- replay states
def replay_state(seed, n, n_ops, L=None, p_held=0.5, p_dup=0.3, p_stale=0.3, p_own=0.33, p_skip=0.05):
    """a frame state with duplicated landmarks, stale outlier entries (with and without a landmark on the view), and ops that hit held views, their
    own view, views of other ops' landmarks and empty views; every landmark in at most one op; ops in shuffled array order, some skipped.  The p_*
    are the densities of held views, duplicates, stale entries on empty views, ops onto their landmark's holder and skipped ops"""
    rng = np.random.default_rng(seed)
    L = L or max(4, (n + n_ops) * 2 // 3)
    kp_lm = np.where(rng.random(n) < p_held, rng.integers(0, L, n), -1).astype(np.int32)
    dup = rng.random(n) < p_dup
    if n > 1:
        kp_lm[dup] = kp_lm[rng.integers(0, n, int(dup.sum()))]
    kp_outl = np.where(kp_lm >= 0, rng.integers(1, 3, n), np.where(rng.random(n) < p_stale, rng.integers(1, 3, n), 0)).astype(np.uint8)
    n_real = min(n_ops, L)
    op_lm = np.full(n_ops, -1, np.int32)
    op_lm[:n_real] = rng.permutation(L)[:n_real]
    op_view = rng.integers(0, n, n_ops).astype(np.int32)
    held = np.nonzero(kp_lm >= 0)[0]
    for j in range(n_real):                                                 # a third of the ops name the view that already holds their landmark
        at = np.nonzero(kp_lm == op_lm[j])[0]
        if len(at) and rng.random() < p_own:
            op_view[j] = at[0] if rng.random() < 0.5 else at[-1]              # the first holder is hasAssociation(lm)'s answer
    op_view[rng.random(n_ops) < p_skip] = -1
    op_lm[rng.random(n_ops) < p_skip] = -1
    return dict(kp_lm=kp_lm, kp_outl=kp_outl, n_matches=int(rng.integers(0, n + 3)), op_view=op_view, op_lm=op_lm, L=L)
