"""Cases for the tracker's first stage with its fall-back (tests/test_refkf_ref.py on the CPU; tests/test_gpu_refkf.py runs their search and replay
on the device): a
track_cases scene at the smallest shapes that still reach every branch (96 keypoints, 160 landmarks), a store of three key frames (the reference key
frame of 80 keypoints sees most of what the frame sees, one is unrelated, one is empty), a synthetic vocabulary with three feature-vector nodes (so
that many views share a node) and a share of words without weight, the last frame's pose, and a dirty entry state for the calls that do not start
with the motion model.  Every generator is a pure function of its named seed.

A case QUALIFIES like a tracking case (track_cases.qualifies): every optimiser problem of the reference chain that runs on three or more edges keeps
its classifications MARGIN away from the thresholds under the seeded summation orders (poseopt_cases.qualify)."""
import functools

import numpy as np

import poseopt_cases as PC
import ref_bow
import ref_refkf as RR
import ref_track as R
import scenes
import track_cases as TC

N, N_LAST, EXTRA, N_KF, KF_N = 96, 64, 64, 3, 80
LEVELS, LEVELSUP = 3, 2
RANDOM_BASE, N_RANDOM = 515151, 8


def build(seed, edit=None, rp=None, tp=None, outliers=0.15, sensor=1, kf_cap=KF_N):
    c = TC.build(seed, n=N, n_last=N_LAST, extra=EXTRA, sensor=sensor, outliers=outliers, tp=tp, n_kf=N_KF)
    rng = np.random.default_rng(seed + 31)
    fr, L, slot = c["frame"], len(c["lms"]), c["slot"]
    tree = scenes.flat_tree(rng, LEVELS, lambda i, lv, m: 3, zero_weight=0.08)
    # the reference key frame: 56 keypoints look at a frame view (its landmark, its descriptor with a few bits flipped, its angle turned by 20 degrees, a
    # tenth of them anywhere); 8 look at a view another keypoint looks at already, holding a landmark the frame does not see; 16 are unrelated
    seen = rng.permutation(N)[:56]
    twins = rng.choice(seen, 8, replace=False)
    unseen = np.setdiff1d(np.arange(L), slot)
    spare = rng.permutation(unseen)
    kf_lm = np.concatenate([slot[seen], spare[:8], np.where(rng.random(16) < 0.5, spare[8:24], -1)]).astype(np.int32)
    src = np.concatenate([seen, twins])
    kdesc = np.concatenate([scenes.flip_bits(rng, fr["desc"][src], rng.integers(0, 10, len(src))), rng.integers(0, 256, (16, 32), dtype=np.uint8)])
    kang = np.concatenate([(fr["kps"]["angle"][src] + 20 + rng.normal(0, 3, len(src)) + (rng.random(len(src)) < 0.1) * rng.uniform(0, 360, len(src))) % 360,
                           rng.uniform(0, 360, 16)]).astype(np.float32)
    order = rng.permutation(KF_N)
    sizes = (40, KF_N, 0)
    total = sum(sizes)
    kps = np.zeros(total, TC.KP_DTYPE)
    kps["angle"] = rng.uniform(0, 360, total).astype(np.float32)
    desc = rng.integers(0, 256, (total, 32), dtype=np.uint8)
    kp_lm = np.full(total, -1, np.int32)
    kp_lm[:40] = rng.permutation(L)[:40]
    kps["angle"][40:40 + KF_N], desc[40:40 + KF_N], kp_lm[40:40 + KF_N] = kang[order], kdesc[order], kf_lm[order]
    word, weight, node = ref_bow.bow_transform(tree, desc, LEVELSUP)
    node = np.where(weight > 0, node, -1).astype(np.int32)                   # `if (w > 0) fv.addFeature(nid, i)`: the caller's part on the key-frame side
    K = dict(n_kf=N_KF, kf_off=np.array([0, 40, 40 + KF_N, total], np.int64), kps=kps, desc=np.ascontiguousarray(desc), node=node, kp_lm=kp_lm)
    # the entry state of a call that does not start with the motion model: views that hold their own landmark (the op finds its view occupied by
    # its own landmark), views that hold the landmark of ANOTHER seen view (the op moves it), views that hold something else, stale flags
    st_lm, st_outl = np.full(N, -1, np.int32), np.zeros(N, np.uint8)
    own, moved, other = seen[:6], seen[6:10], seen[10:13]
    st_lm[own] = slot[own]
    free = np.setdiff1d(np.arange(N), seen)
    st_lm[free[:4]] = slot[moved]
    st_lm[other] = slot[free[4:7]]
    st_outl[st_lm >= 0] = 1
    st_outl[free[8:11]] = (1, 2, 2)
    Tl = c["Tcw_pred"].copy()
    Tl[:3, 3] += np.array([0.02, -0.01, 0.015], np.float32)
    Te = np.eye(4, dtype=np.float32)
    Te[:3, 3] = (1, 2, 3)
    c.update(tree=tree, levelsup=LEVELSUP, K=K, kf_slot=1, kf_cap=kf_cap, Tcw_last=Tl, Tcw_entry=Te, rp=rp or RR.RefKfParams(),
             state0=(st_lm, st_outl, int((st_lm >= 0).sum())), seen=seen)
    if edit:
        edit(c, rng)
    return c


def reference(c, velocity_valid):
    """the dense chain -> (motion or None, refkf, local)"""
    return RR.track_normal_dense(c, velocity_valid, c["state0"])


def qualifies(c, ref):
    motion, refkf, local = ref
    probs = [(refkf, c["Tcw_last"], refkf["status"] == RR.REFKF_OK), (local, refkf["Tcw_init"].reshape(4, 4), True)]
    if motion is not None:
        probs.append((motion, c["Tcw_pred"], motion["status"] == R.TRACK_OK))
    for stage, T_in, run in probs:
        if run and len(stage["edges"]) >= 3 and PC.qualify(T_in, stage["cam"], stage["edges"]) is None:
            return False
    return True


# ---- directed cases: name -> (builder arguments, velocity_valid, what must hold in the reference's result)
def _ref_of(c, vv):
    return RR.track_normal_dense(c, vv, c["state0"])


def _bad_kf_landmarks(c, rng):
    a, b = c["K"]["kf_off"][1:3]
    held = c["K"]["kp_lm"][a:b]
    c["T"]["lm_bad"][held[held >= 0][::6]] = 1


def _bow_gate(delta):
    def edit(c, rng):                                                       # N_min_matches_BoW = the search's count + delta
        n_bow = _ref_of(c, 0)[1]["result"]["n_bow"][0]
        c["rp"] = RR.RefKfParams(n_min_matches_bow=int(n_bow) + delta, thresh_init=c["rp"].thresh_init)
    return edit


def _motion_gate(delta):
    def edit(c, rng):                                                       # thresh_init = the motion model's return value + delta
        m = R.track_motion_model(c["frame"], c["Tcw_pred"], c["last_kps"], c["last_kp_lm"], c["lms"], c["T"]["lm_nobs"], c["tp"], R.DenseMatches(N))
        c["rp"] = RR.RefKfParams(thresh_init=m["n_matches_map"] + delta)
    return edit


def _init_is_thresh(c, rng):                                                # thresh_init = the reference key frame's return value: success is 0
    c["rp"] = RR.RefKfParams(thresh_init=int(_ref_of(c, 0)[1]["result"]["n_matches_map_refkf"][0]))


def _slot(s):
    def edit(c, rng):
        c["kf_slot"] = s
    return edit


def _few_edges(c, rng):                                                     # two matches pass a gate of 2; nothing else is on the frame
    a, b = c["K"]["kf_off"][1:3]
    _, rk, _ = _ref_of(c, 0)
    live = np.nonzero(rk["match_kf"] >= 0)[0]
    c["K"]["kp_lm"][a:b][np.setdiff1d(np.arange(b - a), live[:2])] = -1
    c["state0"] = (np.full(N, -1, np.int32), np.zeros(N, np.uint8), 0)
    c["rp"] = RR.RefKfParams(n_min_matches_bow=2, thresh_init=c["rp"].thresh_init)


def _weak_motion(c, rng):                                                   # the motion model finds too little: the fall-back runs on its leftovers
    held = np.nonzero(c["last_kp_lm"] >= 0)[0]
    c["last_kp_lm"][held[25:]] = -1
    c["rp"] = RR.RefKfParams(thresh_init=40)


def _failed_motion(c, rng):
    held = np.nonzero(c["last_kp_lm"] >= 0)[0]
    c["last_kp_lm"][held[8:]] = -1


OK, FAILED, SKIPPED = RR.REFKF_OK, RR.REFKF_BOW_FAILED, RR.REFKF_SKIPPED


def _collapsed(rk):                                                         # two key-frame keypoints took one view
    f = rk["match_kf"][rk["match_kf"] >= 0]
    return len(f) > len(np.unique(f)) and rk["result"]["n_bow"][0] == len(f) > (rk["op_view"] >= 0).sum()


def _st(rk):
    return int(rk["result"]["refkf_status"][0])


DIRECTED = {
    "plain": (dict(), 0, lambda c, m, rk, l: _st(rk) == OK and rk["pose"]["status"] == 0 and rk["result"]["success"][0] == 1),
    "two_take_one_view": (dict(), 0, lambda c, m, rk, l: _st(rk) == OK and _collapsed(rk)),
    "bad_kf_landmark": (dict(edit=_bad_kf_landmarks), 0, lambda c, m, rk, l: _st(rk) == OK and rk["result"]["n_bow"][0] < _ref_of(build(c["seed"]), 0)[1]["result"]["n_bow"][0]),
    "held_elsewhere": (dict(), 0, lambda c, m, rk, l: _st(rk) == OK and ((c["state0"][0] >= 0) & (rk["after_associate"][0] == -1)).any()),
    "view_occupied": (dict(), 0, lambda c, m, rk, l: _st(rk) == OK and ((c["state0"][0] >= 0) & (rk["op_lm"] >= 0) & (rk["op_lm"] != c["state0"][0])).any()),
    "bow_gate_exact": (dict(edit=_bow_gate(0)), 0, lambda c, m, rk, l: _st(rk) == OK and rk["result"]["n_bow"][0] == c["rp"].n_min_matches_bow),
    "bow_gate_below": (dict(edit=_bow_gate(1)), 0, lambda c, m, rk, l: _st(rk) == FAILED and rk["result"]["n_init"][0] == -1 and rk["n_edges"][1] == 0),
    "bow_gate_below_after_motion": (dict(edit=lambda c, rng: (_weak_motion(c, rng), _bow_gate(1)(c, rng))), 1,
                                    lambda c, m, rk, l: _st(rk) == FAILED and m["status"] == 0 and rk["result"]["success"][0] == 0),
    "motion_gate_exact": (dict(edit=_motion_gate(0)), 1, lambda c, m, rk, l: _st(rk) == SKIPPED and rk["result"]["n_init"][0] == c["rp"].thresh_init),
    "motion_gate_below": (dict(edit=_motion_gate(1)), 1, lambda c, m, rk, l: _st(rk) == OK and m["status"] == 0),
    "fallback_after_weak_motion": (dict(edit=_weak_motion), 1, lambda c, m, rk, l: _st(rk) == OK and m["status"] == 0 and (m["state"][0] >= 0).sum() > 5),
    "fallback_after_failed_motion": (dict(edit=_failed_motion), 1, lambda c, m, rk, l: _st(rk) == OK and m["status"] == 1),
    "skipped": (dict(), 1, lambda c, m, rk, l: _st(rk) == SKIPPED and rk["result"]["success"][0] == 1 and rk["result"]["n_bow"][0] > 0),
    "init_is_thresh": (dict(edit=_init_is_thresh), 0, lambda c, m, rk, l: _st(rk) == OK and rk["result"]["n_init"][0] == c["rp"].thresh_init and rk["result"]["success"][0] == 0),
    "slot_minus_one": (dict(edit=_slot(-1)), 0, lambda c, m, rk, l: _st(rk) == FAILED and rk["result"]["n_bow"][0] == 0 and (rk["match_kf"] == -1).all()),
    "slot_past_the_store": (dict(edit=_slot(N_KF)), 0, lambda c, m, rk, l: _st(rk) == FAILED and rk["result"]["n_bow"][0] == 0),
    "empty_keyframe": (dict(edit=_slot(2)), 0, lambda c, m, rk, l: _st(rk) == FAILED and rk["result"]["n_bow"][0] == 0),
    "kf_cap_truncates": (dict(kf_cap=50), 0, lambda c, m, rk, l: _st(rk) == OK and 0 < rk["result"]["n_bow"][0] < _ref_of(build(c["seed"]), 0)[1]["result"]["n_bow"][0]),
    "too_few_edges": (dict(edit=_few_edges), 0, lambda c, m, rk, l: _st(rk) == OK and rk["pose"]["status"] == 1 and 0 < rk["n_edges"][0] < 3),
    "mono": (dict(sensor=0), 0, lambda c, m, rk, l: _st(rk) == OK and rk["pose"]["status"] == 0),
}
DIRECTED_BASE = {name: 70001 + 1000 * k for k, name in enumerate(DIRECTED)}


@functools.lru_cache(maxsize=None)
def directed(name):
    """-> (case, velocity_valid, (motion, refkf, local)) of the first seed whose reference result has the directed property and qualifies"""
    args, vv, holds = DIRECTED[name]
    for seed in range(DIRECTED_BASE[name], DIRECTED_BASE[name] + 40):
        c = build(seed, **args)
        ref = reference(c, vv)
        if holds(c, *ref) and qualifies(c, ref):
            return c, vv, ref
    raise AssertionError("no qualifying seed for " + name)


@functools.lru_cache(maxsize=None)
def random_cases():
    """-> ([(case, velocity_valid, reference)], seeds drawn): seeds from RANDOM_BASE on until N_RANDOM qualify; at least three quarters must.  The
    velocity is valid on every other seed; a third of those have a weak motion model, so that the fall-back runs"""
    out, drawn = [], 0
    while len(out) < N_RANDOM:
        vv = drawn % 2
        c = build(RANDOM_BASE + drawn, edit=_weak_motion if drawn % 6 == 1 else None, sensor=1 if drawn % 3 else 0)
        drawn += 1
        ref = reference(c, vv)
        if qualifies(c, ref):
            out.append((c, vv, ref))
        assert 3 * drawn <= 4 * N_RANDOM, "more than a quarter of the drawn seeds rejected"
    return out, drawn


# ---- replay states for the view-order replay: a view in at most one op, a landmark in at most one
def replay_state(seed, n, L=None, p_own=0.33, p_skip=0.03, **state):
    """TC.replay_state's frame state (`state`: its densities) with ops that name every view and every landmark at most once"""
    rng = np.random.default_rng(seed)
    s = TC.replay_state(seed, n, n, L, **state)
    L = s["L"]
    views = rng.permutation(n)
    k = int(min(n, L) * rng.uniform(0.3, 1.0))
    op_view, op_lm = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    lms = rng.permutation(L)[:k]
    for j in range(k):                                                      # a third of the ops name a view that already holds their landmark
        at = np.nonzero(s["kp_lm"] == lms[j])[0]
        if len(at) and rng.random() < p_own and at[0] not in op_view:
            op_view[j] = at[0] if rng.random() < 0.5 or at[-1] in op_view else at[-1]
        else:
            free = views[~np.isin(views, op_view)]
            op_view[j] = free[0]
        op_lm[j] = lms[j]
    op_view[rng.random(n) < p_skip] = -1                                     # skipped ops
    op_lm[rng.random(n) < p_skip] = -1
    p = rng.permutation(n)
    return dict(kp_lm=s["kp_lm"], kp_outl=s["kp_outl"], n_matches=s["n_matches"], op_view=op_view[p], op_lm=op_lm[p], L=L)


def random_search(seed, n, kf_sizes, L, n_nodes, p_lm=0.9, p_bad=0.05, p_twin=0.3, p_turned=0.15, max_flip=14, p_no_node=0.05):
    """inputs of the key-frame / frame BoW search without a vocabulary: a frame of n keypoints with random descriptors, angles and nodes, and a store
    of key frames with kf_sizes keypoints each, every one a copy of a frame keypoint (with repeats: twins that compete for one view) with up to
    max_flip bits flipped, its node and its angle, a share turned away (the rotation histogram removes those).  Some keypoints have no node or no
    weight, on both sides.  -> (K, lm_bad, fkps, fdesc, fnode, fweight)"""
    rng = np.random.default_rng(seed)
    fdesc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    fkps = np.zeros(n, TC.KP_DTYPE)
    fkps["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    fnode = np.where(rng.random(n) < p_no_node, -1, rng.integers(0, max(n_nodes, 1), n)).astype(np.int32)
    fweight = np.where(rng.random(n) < p_no_node, 0.0, rng.uniform(0.1, 3, n)).astype(np.float32)
    off = np.zeros(len(kf_sizes) + 1, np.int64)
    np.cumsum(kf_sizes, out=off[1:])
    total = int(off[-1])
    src = rng.integers(0, n, total)
    twin = rng.random(total) < p_twin
    if total > 1:
        src[1:][twin[1:]] = src[:-1][twin[1:]]
    K = dict(n_kf=len(kf_sizes), kf_off=off, kps=np.zeros(total, TC.KP_DTYPE), desc=scenes.flip_bits(rng, fdesc[src], rng.integers(0, max_flip + 1, total)),
             kp_lm=np.where(rng.random(total) < p_lm, rng.integers(0, max(L, 1), total), -1).astype(np.int32))
    K["kps"]["angle"] = ((fkps["angle"][src] + 300 + rng.normal(0, 4, total) + (rng.random(total) < p_turned) * rng.uniform(0, 360, total)) % 360).astype(np.float32)
    K["node"] = np.where(rng.random(total) < p_no_node, -1, fnode[src]).astype(np.int32)
    return K, (rng.random(L) < p_bad).astype(np.uint8), fkps, fdesc, fnode, fweight
