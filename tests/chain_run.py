"""Runs of frames for the resident chain (tests/test_chain_run_ref.py on the CPU, tests/test_gpu_chain_run.py on the device): the frames a SLAM loop
would push through ONE set of caller-owned buffers (d_work, hs_track_state, hs_track_out, hs_keyframe_out, the entry update's outputs), with n, n_last,
L, cap, new_cap and the outcome changing from frame to frame.  The tracking cases are those of track_cases as they are (build / directed) with
keyframe_cases' key-frame stores; this module only picks them, puts them in order and says what each frame's later stages are fed.  refkf_cases.build
has fixed sizes, so the frames of the reference-key-frame run are made here in its style, with its replay states (refkf_frame).

A slot takes the first seed, within DRAWS draws from its base, whose reference result has the slot's property and which track_cases.qualifies (the
rule of track_cases.directed).  A slot without such a seed raises; nothing is skipped or dropped.

  A  narrow window, mid size                 n = 300, n_last = 200, L = 400
  B  below one wave                          the smallest n <= 64 (n_last = 2n/3 < n, L = n + n/3 < 128) for which a seed qualifies: B_N
  C  wide window                             DIRECTED["wide"]
  D  motion stage fails, gate closes         DIRECTED["both_fail"]: the later stages do not run
  E  past 1024 views and 1024 landmarks      DIRECTED["chunk_1025"]
  F  the optimiser does not run              DIRECTED["too_few_edges"]
  G  mono after stereo, just over a block    sensor 0, n = 257, n_last = 130, L = 320
  H  G's scene one step later                the last frame is G itself: its keypoints, its final associations, its final pose
  I  A again                                 the very object of slot A

After every frame whose reference track status is OK come hs_track_keyframe_device and hs_landmark_update_entries_device; the parameter sets
alternate between not inserting and inserting (force = 1) over those frames in table order, starting with not inserting."""
import functools

import numpy as np

import keyframe_cases as KC
import ref_keyframe as RKF
import ref_refkf as RR
import ref_track as R
import refkf_cases as RC
import scenes
import ref_bow
import track_cases as TC

DRAWS = 40
SLOTS = "ABCDEFGHI"
B_N = 33                                                                     # found by smallest_b() on the CPU (n_last = 22, L = 44; seed 62007); test_chain_run_ref.py holds it to that
BASE = dict(A=61001, B=62001, G=67001)
ARGS = dict(A=dict(n=300, n_last=200, extra=100), G=dict(sensor=0, n=257, n_last=130, extra=63))
# the orders the device runs: the table's, backwards, starting from E, and ascending n with the rest behind (the arena regrows while frames are queued).
# G and H stay a pair in every order: H is defined by what G left on the device
ORDERS = dict(table="ABCDEFGHI", reverse="IGHFEDCBA", rotated="EFGHIABCD", ascending="BGHACDFEI")


def b_args(n):
    return dict(n=n, n_last=2 * n // 3, extra=n // 3)


def _ok(m, l):
    return m["status"] == R.TRACK_OK


PROPERTY = dict(A=TC.DIRECTED["narrow"][1], B=_ok, C=TC.DIRECTED["wide"][1], D=TC.DIRECTED["both_fail"][1], E=TC.DIRECTED["chunk_1025"][1],
                F=TC.DIRECTED["too_few_edges"][1], G=_ok, H=_ok)


def first_seed(base, args, holds):
    """-> (case, reference) of the first of DRAWS seeds from `base` with the property that qualifies, or None"""
    for seed in range(base, base + DRAWS):
        c = TC.build(seed, **args)
        ref = TC.reference(c)
        if holds(*ref) and TC.qualifies(c, ref):
            return c, ref
    return None


def smallest_b(lo=4):
    """the search B_N records: ascending n, the first for which a seed resolves"""
    for n in range(lo, 65):
        if first_seed(BASE["B"], b_args(n), _ok) is not None:
            return n
    raise AssertionError("no n <= 64 resolves slot B")


class Frame:
    """one frame of a run: the tracking case, its reference, and what the later stages are fed (kf: None when they do not run)"""

    def __init__(self, slot, c, ref, insert):
        self.slot, self.c, self.ref = slot, c, ref
        self.n, self.n_last, self.L, self.cap, self.n_kf = len(c["frame"]["kps"]), len(c["last_kp_lm"]), len(c["lms"]), c["cap"], len(c["T"]["kf_id"])
        self.kf = keyframe_inputs(c, insert) if ref[0]["status"] == R.TRACK_OK else None
        self.new_cap = self.kf["new_cap"] if self.kf else 0


def keyframe_inputs(c, insert):
    """depth from the stereo coordinate, a store of key frames of 70 keypoints, new_cap = n (test_chain_track_then_keyframe_then_entry_update's)"""
    fr, L, n = c["frame"], len(c["lms"]), len(c["frame"]["kps"])
    with np.errstate(all="ignore"):
        depth = np.where(fr["uR"] > 0, np.float32(fr["mbf"]) / (fr["kps"]["x"] - fr["uR"]).astype(np.float32), np.float32(-1)).astype(np.float32)
    rng = np.random.default_rng(4)
    K = KC.keyframes([rng.integers(-1, L, 70).tolist() for _ in range(len(c["T"]["kf_id"]))])
    th = float(np.median(depth[depth > 0])) if (depth > 0).any() else 40.0
    common = dict(th_depth=th, n_min_points=20, thresh_init=5, thresh_refine=5)
    quiet = dict(frame_id=12, last_keyframe_id=10, N_tracked_target=0, N_tracked_variance=0, min_N_tracked_close=0)       # nothing asks for a key frame
    return dict(depth=depth, K=K, prm=RKF.params(**common, **(dict(force=1) if insert else quiet)), new_cap=n, insert=insert)


def keyframe_case(f, state, Tcw, track):
    """the case ref_keyframe.literal takes, from the state, pose and result the tracking chain left (the reference's or the device's)"""
    return dict(state=(np.asarray(state[0], np.int32), np.asarray(state[1], np.uint8), int(state[2])), T=f.c["T"], K=f.kf["K"], depth=f.kf["depth"], frame=f.c["frame"],
                Tcw=np.asarray(Tcw, np.float32).reshape(4, 4), track=dict(track), prm=f.kf["prm"], ref_slot=-1, new_cap=f.kf["new_cap"])


def keyframe_reference(f):
    """ref_keyframe.literal after the REFERENCE's tracking result of frame f"""
    m, l = f.ref
    return RKF.literal(keyframe_case(f, l["state"], l["pose"]["Tcw"], dict(status=m["status"], n_matches_map=m["n_matches_map"], n_inliers=l["n_inliers"])))


def derive_h(g, kp_lm_final, Tcw_final):
    """slot H from frame G's final associations and final pose: -> (case, reference, qualifies and tracks)"""
    c = dict(g.c, last_kps=g.c["frame"]["kps"], last_kp_lm=np.ascontiguousarray(kp_lm_final, np.int32), Tcw_pred=np.asarray(Tcw_final, np.float32).reshape(4, 4).copy())
    ref = TC.reference(c)
    return c, ref, bool(PROPERTY["H"](*ref) and TC.qualifies(c, ref))


@functools.lru_cache(maxsize=None)
def run():
    """-> {slot: Frame}; slot I is slot A's Frame"""
    picked = {}
    for slot in "ABCDEFG":
        if slot in "CDEF":
            picked[slot] = TC.directed({"C": "wide", "D": "both_fail", "E": "chunk_1025", "F": "too_few_edges"}[slot])
        else:
            got = first_seed(BASE[slot], b_args(B_N) if slot == "B" else ARGS[slot], PROPERTY[slot])
            assert got is not None, "no qualifying seed for slot " + slot
            picked[slot] = got
    frames, insert = {}, False
    for slot in "ABCDEFG":
        c, ref = picked[slot]
        assert PROPERTY[slot](*ref), slot
        frames[slot] = Frame(slot, c, ref, insert)
        if frames[slot].kf:
            insert = not insert
    g = frames["G"]
    assert g.kf is not None
    c, ref, ok = derive_h(g, keyframe_reference(g)["kp_lm"], g.ref[1]["pose"]["Tcw"])
    assert ok, "slot H, built from the reference's result of G, does not qualify"
    frames["H"] = Frame("H", c, ref, insert)
    frames["I"] = frames["A"]
    return frames


def ordered(order):
    fr = run()
    return [fr[s] for s in ORDERS[order]]


# ---------------------------------------------------------------- the reference-key-frame run
REFKF_VIEWS = (130, 5, 1025, 64, 257)
REFKF_BASE = 81001


def refkf_frame(n, k):
    """frame k of the refkf run: a refkf_cases-style scene at n views (the builder's own construction needs its fixed 96; this is the search's and
    the replay's input at other sizes, as test_search_by_bow_kf_beyond_one_pass makes it): a key frame of nk keypoints that look at frame views, a store
    of three key frames, kf_cap below, at and above nk in turn, a dirty entry state from refkf_cases.replay_state"""
    rng = np.random.default_rng(REFKF_BASE + n)
    nk, L = max(3, (4 * n) // 5), 2 * n + 8
    tree = scenes.flat_tree(rng, RC.LEVELS, lambda i, lv, m: 3, zero_weight=0.08)
    fdesc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    fkps = np.zeros(n, TC.KP_DTYPE)
    fkps["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    src = rng.integers(0, n, nk)                                             # with repeats: two key-frame keypoints take one view
    total = 3 + nk
    K = dict(n_kf=3, kf_off=np.array([0, 3, total, total], np.int64), kps=np.zeros(total, TC.KP_DTYPE), desc=rng.integers(0, 256, (total, 32), dtype=np.uint8),
             kp_lm=np.full(total, -1, np.int32))
    K["desc"][3:] = scenes.flip_bits(rng, fdesc[src], rng.integers(0, 10, nk))
    K["kps"]["angle"][3:] = ((fkps["angle"][src] + 20 + rng.normal(0, 3, nk) + (rng.random(nk) < 0.1) * rng.uniform(0, 360, nk)) % 360).astype(np.float32)
    K["kp_lm"][3:] = np.where(rng.random(nk) < 0.9, rng.permutation(L)[:nk], -1)
    _, wt, nd = ref_bow.bow_transform(tree, K["desc"], RC.LEVELSUP)
    K["node"] = np.where(wt > 0, nd, -1).astype(np.int32)
    _, fwt, fnd = ref_bow.bow_transform(tree, fdesc, RC.LEVELSUP)
    node = np.where(fwt > 0, fnd, -1).astype(np.int32)
    lm_bad = (rng.random(L) < 0.05).astype(np.uint8)
    kf_cap = (max(nk - 2, 1), nk, nk + 7)[k % 3]
    s0 = RC.replay_state(REFKF_BASE + 500 + n, n, L)
    search = RR.search_by_bow_kf_dense(K, 1, kf_cap, L, lm_bad, fkps, fdesc, node, None, 50.0, 0.8)        # (match_kf, op_view, op_lm, n_matches)
    want = RR.replay_views_sequential(R.MapMatches.from_dense(s0["kp_lm"], s0["kp_outl"], s0["n_matches"]), search[1], search[2], n, L).dense(n)
    return dict(n=n, nk=nk, L=L, kf_cap=kf_cap, K=K, kf_slot=1, kps=fkps, desc=fdesc, node=node, lm_bad=lm_bad, state0=(s0["kp_lm"], s0["kp_outl"], s0["n_matches"]),
                search=search, state=want, th_low=50.0, nnratio=0.8)


@functools.lru_cache(maxsize=None)
def refkf_run():
    return [refkf_frame(n, k) for k, n in enumerate(REFKF_VIEWS)]
