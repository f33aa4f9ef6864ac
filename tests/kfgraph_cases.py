"""Inputs for the key-frame graph tests (tests/ref_kfgraph.py, hs_kf_votes / hs_kf_redundancy): random observation tables, queries and culler
candidates, and small cases whose answers are derived by hand from the reference's text."""
import numpy as np


def table(n_kf, observations, lm_bad=None, lm_nobs=None, kf_bad=None, kf_id=None):
    """observations: per landmark a list of slots (octave 0) or of (slot, octave) pairs, ascending slots"""
    rows = [[(o, 0) if np.isscalar(o) else tuple(o) for o in obs] for obs in observations]
    L = len(rows)
    off = np.zeros(L + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    flat = np.array([p for r in rows for p in r], np.int32).reshape(-1, 2)
    return dict(lm_obs_offsets=off, lm_obs_kf=np.ascontiguousarray(flat[:, 0]), lm_obs_octave=np.ascontiguousarray(flat[:, 1]),
                lm_bad=np.zeros(L, np.uint8) if lm_bad is None else np.asarray(lm_bad, np.uint8),
                lm_nobs=np.diff(off).astype(np.int32) if lm_nobs is None else np.asarray(lm_nobs, np.int32),
                kf_bad=np.zeros(n_kf, np.uint8) if kf_bad is None else np.asarray(kf_bad, np.uint8),
                kf_id=np.arange(n_kf, dtype=np.int64) if kf_id is None else np.asarray(kf_id, np.int64))


def csr(lists, dtype=np.int32):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.concatenate([np.asarray(x, dtype).reshape(-1) for x in lists]) if lists else np.zeros(0, dtype)
    return off, np.ascontiguousarray(flat.astype(dtype))


def random_table(seed, n_kf, L, max_obs=40, big=(), window=False, p_bad_lm=0.05, p_bad_kf=0.05):
    """L landmarks with 0 .. min(max_obs, n_kf) observations each (`big`: (landmark, count) overrides); window=True: a landmark is seen by a run of
    consecutive key frames, as a map grows; otherwise by a random subset.  kf_id: a permutation with one id carried by two slots."""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, min(max_obs, n_kf) + 1, L)
    for lm, cnt in big:
        n[lm] = min(cnt, n_kf)
    off = np.zeros(L + 1, np.int64)
    np.cumsum(n, out=off[1:])
    owner = np.repeat(np.arange(L), n)
    within = np.arange(int(off[-1])) - off[owner]
    if window:
        start = rng.integers(0, n_kf, L)
        start = np.minimum(start, n_kf - n)
        kf = (start[owner] + within).astype(np.int32)
    else:
        kf = np.zeros(int(off[-1]), np.int32)
        for i in range(L):
            kf[off[i]:off[i + 1]] = np.sort(rng.choice(n_kf, int(n[i]), replace=False))
    kf_id = rng.permutation(n_kf).astype(np.int64) + 100
    if n_kf > 3:
        kf_id[n_kf - 1] = kf_id[1]
    return dict(lm_obs_offsets=off, lm_obs_kf=kf, lm_obs_octave=rng.integers(0, 8, len(kf)).astype(np.int32),
                lm_bad=(rng.random(L) < p_bad_lm).astype(np.uint8), lm_nobs=(n + rng.integers(0, 2, L) * rng.integers(0, n + 1)).astype(np.int32),
                kf_bad=(rng.random(n_kf) < p_bad_kf).astype(np.uint8), kf_id=kf_id)


def key_frame_queries(T):
    """a whole-graph recompute: query s = the landmarks key frame s observes (pKF->GetMapPoints()), self id = its mnId"""
    n_kf, L = len(T["kf_id"]), len(T["lm_bad"])
    owner = np.repeat(np.arange(L), np.diff(T["lm_obs_offsets"]))
    order = np.lexsort((owner, T["lm_obs_kf"]))
    q_lm = owner[order].astype(np.int32)
    off = np.zeros(n_kf + 1, np.int64)
    np.cumsum(np.bincount(T["lm_obs_kf"], minlength=n_kf), out=off[1:])
    return off, q_lm, T["kf_id"].copy()


def random_candidates(seed, T, sizes):
    """culler candidates with `sizes` items each: random landmarks, octaves and depths (some negative, some beyond mThDepth)"""
    rng = np.random.default_rng(seed)
    L, n_kf = len(T["lm_bad"]), len(T["kf_id"])
    off = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(sizes, out=off[1:])
    n = int(off[-1])
    depth = rng.uniform(-2, 50, n).astype(np.float32)
    return dict(cand_slot=rng.integers(0, n_kf, len(sizes)).astype(np.int32), cand_th_depth=rng.uniform(20, 45, len(sizes)).astype(np.float32),
                cand_offsets=off, item_lm=rng.integers(0, max(L, 1), n).astype(np.int32), item_octave=rng.integers(0, 8, n).astype(np.int32),
                item_depth=depth)


# ---- votes: (table, queries, self ids, count_bad_kf, th, cap) -> expected outputs, derived by hand
_T4 = table(4, [[1, 2], [1, 2], [0, 1, 2, 3]])
_TID = table(4, [[0, 1, 2, 3]], kf_id=[7, 5, 7, 9])
_TBAD = table(3, [[0, 1], [1], [1, 2]], kf_bad=[0, 1, 0])
_TLM = table(3, [[0, 1], [1, 2]], lm_bad=[1, 1])

KNOWN_VOTES = {
    # two key frames share both landmarks: `if (count > nmax)` on ascending slots keeps slot 1; nothing reaches th = 3: the single (nmax, pKFmax) entry
    "max_tie_lowest_slot_and_fallback": dict(T=_T4, queries=[[0, 1]], self_id=[-1], count_bad_kf=0, th=3, cap=4,
                                             weights=[[0, 2, 2, 0]], max_slot=[1], max_count=[2], n_ordered=[1],
                                             ordered_slot=[[1, -1, -1, -1]], ordered_weight=[[2, 0, 0, 0]]),
    # sort(vPairs) is ascending in (weight, pointer), push_front reverses it: among equal weights the HIGHER slot comes first
    "ordered_ties_higher_slot_first": dict(T=_T4, queries=[[0, 1, 2]], self_id=[-1], count_bad_kf=0, th=1, cap=4,
                                           weights=[[1, 3, 3, 1]], max_slot=[1], max_count=[3], n_ordered=[4],
                                           ordered_slot=[[2, 1, 3, 0]], ordered_weight=[[3, 3, 1, 1]]),
    # the same list through cap = 2 (truncated, n_ordered keeps the full length) and cap = 6 (padded with -1 / 0)
    "cap_smaller": dict(T=_T4, queries=[[0, 1, 2]], self_id=[-1], count_bad_kf=0, th=1, cap=2,
                        weights=[[1, 3, 3, 1]], max_slot=[1], max_count=[3], n_ordered=[4], ordered_slot=[[2, 1]], ordered_weight=[[3, 3]]),
    "cap_larger": dict(T=_T4, queries=[[0, 1, 2]], self_id=[-1], count_bad_kf=0, th=1, cap=6,
                       weights=[[1, 3, 3, 1]], max_slot=[1], max_count=[3], n_ordered=[4],
                       ordered_slot=[[2, 1, 3, 0, -1, -1]], ordered_weight=[[3, 3, 1, 1, 0, 0]]),
    # no landmark, and only bad landmarks: KFcounter.empty(), the reference returns
    "empty_counter": dict(T=_TLM, queries=[[], [0, 1]], self_id=[-1, -1], count_bad_kf=0, th=1, cap=2,
                          weights=[[0, 0, 0], [0, 0, 0]], max_slot=[-1, -1], max_count=[0, 0], n_ordered=[0, 0],
                          ordered_slot=[[-1, -1], [-1, -1]], ordered_weight=[[0, 0], [0, 0]]),
    # mnId 7 is carried by slots 0 and 2: `pKF_obs->mnId == pKF_node->mnId` leaves both out
    "self_excluded_by_id": dict(T=_TID, queries=[[0]], self_id=[7], count_bad_kf=0, th=1, cap=3,
                                weights=[[0, 1, 0, 1]], max_slot=[1], max_count=[1], n_ordered=[2],
                                ordered_slot=[[3, 1, -1]], ordered_weight=[[1, 1, 0]]),
    # UpdateLocalKeyFrames counts the bad key frame 1 (3 votes) but `if (pKF->isBad()) continue` keeps it from being chosen or listed
    "bad_kf_counted_not_chosen": dict(T=_TBAD, queries=[[0, 1, 2]], self_id=[-1], count_bad_kf=1, th=1, cap=3,
                                      weights=[[1, 3, 1]], max_slot=[0], max_count=[1], n_ordered=[2],
                                      ordered_slot=[[2, 0, -1]], ordered_weight=[[1, 1, 0]]),
    # covisibility never counts it
    "bad_kf_not_counted": dict(T=_TBAD, queries=[[0, 1, 2]], self_id=[-1], count_bad_kf=0, th=1, cap=3,
                               weights=[[1, 0, 1]], max_slot=[0], max_count=[1], n_ordered=[2],
                               ordered_slot=[[2, 0, -1]], ordered_weight=[[1, 1, 0]]),
    # a landmark listed twice counts twice
    "duplicates_count_twice": dict(T=_T4, queries=[[0, 0, 2]], self_id=[-1], count_bad_kf=0, th=3, cap=2,
                                   weights=[[1, 3, 3, 1]], max_slot=[1], max_count=[3], n_ordered=[2],
                                   ordered_slot=[[2, 1]], ordered_weight=[[3, 3]]),
}

# ---- redundancy.  Landmarks: 0: three other observers at octaves 3, 3, 3 and Observations() = 4;  1: the same with Observations() = 3 (== th_obs: not
# considered);  2: octaves 3, 3, 4 (one fails `<= 2 + 1`);  3: bad;  4: observed by the candidate itself (slot 0) and three others at octave 0
_TR = table(5, [[(1, 3), (2, 3), (3, 3)], [(1, 3), (2, 3), (3, 3)], [(1, 3), (2, 3), (3, 4)], [(1, 0), (2, 0), (3, 0)],
                [(0, 0), (1, 0), (2, 0), (3, 0)]], lm_bad=[0, 0, 0, 1, 0], lm_nobs=[4, 3, 4, 6, 4])


def _cand(items, slot=0, th_depth=10.0):
    return dict(cand_slot=[slot], cand_th_depth=[th_depth], items=[items])


KNOWN_REDUNDANCY = {
    # both items fail `depth_pt > mThDepth || depth_pt < 0`: nMPs = 0, and 0 > 0.9f * 0 is false
    "stereo_depth_gate_and_no_mps": dict(_cand([(0, 2, 10.5), (0, 2, -1.0)]), is_mono=0, th_obs=3, frac=0.9, n_mps=[0], n_redundant=[0], cull=[0]),
    # mono never reads the depth
    "mono_ignores_depth": dict(_cand([(0, 2, 10.5), (0, 2, -1.0)]), is_mono=1, th_obs=3, frac=0.9, n_mps=[2], n_redundant=[2], cull=[1]),
    # Observations() == th_obs is not `> thObs`; th_obs + 1 is
    "nobs_at_and_above_th": dict(_cand([(1, 2, 1.0), (0, 2, 1.0)]), is_mono=0, th_obs=3, frac=0.9, n_mps=[2], n_redundant=[1], cull=[0]),
    # octave 3 passes `<= 2 + 1`, octave 4 does not: landmark 2 has two comparable observers only
    "octave_gate_at_plus_one": dict(_cand([(0, 2, 1.0), (2, 2, 1.0)]), is_mono=0, th_obs=3, frac=0.9, n_mps=[2], n_redundant=[1], cull=[0]),
    # at item octave 1 none of landmark 0's observers (octave 3) is comparable
    "octave_gate_below": dict(_cand([(0, 1, 1.0)]), is_mono=0, th_obs=3, frac=0.9, n_mps=[1], n_redundant=[0], cull=[0]),
    # the bad landmark is not even an nMPs; the candidate's own observation of landmark 4 does not count, the three others do
    "bad_landmark_and_own_observation": dict(_cand([(3, 0, 1.0), (4, 0, 1.0)]), is_mono=0, th_obs=3, frac=0.9, n_mps=[1], n_redundant=[1], cull=[1]),
    # ... seen from slot 4 all four observers of landmark 4 count
    "other_candidate_counts_all": dict(_cand([(4, 0, 1.0)], slot=4), is_mono=0, th_obs=3, frac=0.9, n_mps=[1], n_redundant=[1], cull=[1]),
    # exactly on the verdict: 1 > 0.5f * 2 is false
    "verdict_on_the_boundary": dict(_cand([(0, 2, 1.0), (1, 2, 1.0)]), is_mono=0, th_obs=3, frac=0.5, n_mps=[2], n_redundant=[1], cull=[0]),
    # 9 of 10 at 0.9f: the FLOAT product 0.9f * 10.0f rounds to 9.0f, so 9 > 9.0f is false (in real numbers 9 > 8.9999998 would cull)
    "verdict_float_product": dict(_cand([(0, 2, 1.0)] * 9 + [(1, 2, 1.0)]), is_mono=0, th_obs=3, frac=0.9, n_mps=[10], n_redundant=[9], cull=[0]),
    "verdict_culls": dict(_cand([(0, 2, 1.0)] * 19 + [(1, 2, 1.0)]), is_mono=0, th_obs=3, frac=0.9, n_mps=[20], n_redundant=[19], cull=[1]),
}
KNOWN_REDUNDANCY_TABLE = _TR
