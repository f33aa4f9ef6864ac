#!/usr/bin/env python3
"""Randomised parity sweep of the map-side subsystems (runs on the GPU box): the generators of tests/*_cases.py with their OWN parameters drawn at
random — sizes (extra weight on 0, 1 and k*64 +- 1, k*256 +- 1, k*1024 +- 1), densities, duplicate rates, caps below / at / above the result count,
host or device form, caller stream or the handle's — every case on the device, bit for bit against the independent references of tests/ref_*.py.

    python3 tools/fuzz_map.py --family NAME|all --cases 40 --seed 1          (exit code 1 on the first mismatch)
    python3 tools/fuzz_map.py --family replay --exhaustive 4 4               (both replays over EVERY state and op set of n x L, concatenated)
    python3 tools/fuzz_map.py --family keyframe --exhaustive                 (the three exhaustive spaces of tests/test_keyframe_ref.py, stage by stage)
    python3 tools/fuzz_map.py --tags                                         (generator + reference only, no device: how often each tag is reached)

A family is four functions: draw(rng, i) -> case (generator and reference only, every random number is drawn here), reference(case) -> (want,
reached), device(ctx, case) -> got, and the shared compare(want, got).  `reached` is a set of branch tags computed from the case and the reference's
result alone.  Every drawn case is compared: there is no skip path.  tests/test_fuzz_map_cases.py holds the sweep to its word on the CPU (every tag
reached by the committed slices, a planted mismatch reported), tests/test_gpu_fuzz_map.py runs the slices on the device.

Only inputs that include/hyslam_amd.h says an entry point accepts are passed: the device forms check nothing, so an index outside a table appears
only where the header documents it as skipped.  Left out on purpose: the pose optimiser and every chain that contains it (compared within 1 ulp and
only on qualifying cases: a random sweep would need a skip path), the fused hs_local_map_search_device (tools/fuzz_matchers.py sweeps its search
half), extraction and the matchers (tools/fuzz_parity.py, tools/fuzz_matchers.py)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import keyframe_cases as KF                     # noqa: E402
import kfgraph_cases as KC                      # noqa: E402
import landmark_entry_cases as LE               # noqa: E402
import localmap_cases as LC                     # noqa: E402
import place_cases as PL                        # noqa: E402
import ref_keyframe as RKF                      # noqa: E402
import ref_kfgraph as RK                        # noqa: E402
import ref_landmark as RL                       # noqa: E402
import ref_landmark_entry as RE                 # noqa: E402
import ref_localmap as RLM                      # noqa: E402
import ref_place as RP                          # noqa: E402
import ref_refkf as RR                          # noqa: E402
import refkf_cases as RC                        # noqa: E402
import test_refkf_ref as VR                     # noqa: E402  (seq_batch / state_tables of the view-order replay)
import test_track_ref as LR                     # noqa: E402  (... of the landmark-order replay)
import track_cases as TC                        # noqa: E402

HS_KF_LDS_SLOTS, HS_KF_SORT_PASS, LM_SMALL = 12288, 1024, 64          # include/hyslam_amd.h; kernels_landmark.hip's wave path (the GPU slices check the first two)


# ---------------------------------------------------------------- drawing
def draw_size(rng, hi, lo=0):
    """a size in [lo, hi]: a third uniform, the rest from 0, 1 and k*64 +- 1, k*256 +- 1, k*1024 +- 1"""
    if rng.random() < 0.35:
        return int(rng.integers(lo, hi + 1))
    unit = int(rng.choice([64, 256, 1024]))
    edges = [0, 1, 2] + [k * unit + d for k in range(1, hi // unit + 2) for d in (-1, 0, 1)]
    edges = [e for e in edges if lo <= e <= hi] or [lo]
    return int(edges[int(rng.integers(0, len(edges)))]) if rng.random() < 0.7 else int(rng.choice([e for e in (0, 1, 2, lo) if lo <= e <= hi] or [lo]))


def draw_cap(rng, count):
    """a capacity below, at or above `count`"""
    return max(0, int(count + rng.choice([-5, -1, 0, 0, 1, 7])))


def params(**kw):
    return " ".join("%s=%s" % (k, v) for k, v in kw.items())


# ---------------------------------------------------------------- comparing
def compare(want, got):
    """bit for bit: -> (good, [names of the arrays that differ]).  Integers by value (the references count in int64), floats (float32) by their bits,
    except that a NaN only has to meet a NaN: sign and payload are not specified"""
    bad = []
    for k, w in want.items():
        w, g = np.asarray(w), np.asarray(got[k])
        if w.dtype.kind == "f":
            same = g.dtype == w.dtype and g.shape == w.shape and bool(((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))).all())
        else:
            same = g.shape == w.shape and np.array_equal(w, g)
        if not same:
            bad.append(k)
    return not bad, bad


class HandleStream:
    """the handle's own stream as the device helpers take a stream: .ptr = 0 selects it"""
    ptr = 0

    def __init__(self, ex):
        self._ex = ex

    def synchronize(self):
        self._ex.synchronize()


class Context:
    """the device side, made on first use: one extractor handle, a matcher and a tracker on it, one caller stream"""

    def __init__(self, seed=0):
        self.seed = seed
        self._made = None

    def _make(self):
        if self._made is None:
            import hipmem
            import hyslam_amd as HS
            ex = HS.ORBExtractor(device=0)
            self._made = dict(ex=ex, matcher=HS.FeatureMatcher(extractor=ex), tracker=HS.FrameTracker(ex), own=hipmem.Stream(), handle=HandleStream(ex))
        return self._made

    def __getattr__(self, k):
        return self._make()[k]

    def stream(self, caller):
        return self.own if caller else self.handle


# ================================================================ replay: hs_frame_associate_device, hs_frame_associate_views_device
REPLAY_TAGS = ["fresh insert", "replace", "another view erased", "op on its own holder", "duplicated holder", "stale flag kept", "skipped op"]
REPLAY_OUT = ("kp_lm", "kp_outl", "n_matches")


def _invalid_ops(rng, s, n):
    """some of the skipped ops name an index OUTSIDE the tables instead of -1: the header documents both as skipped"""
    for k, bound in (("op_view", n), ("op_lm", s["L"])):
        at = np.nonzero(s[k] < 0)[0]
        at = at[rng.random(len(at)) < 0.5]
        s[k][at] = rng.choice(np.array([bound, bound + 1, bound + 4097, 2 ** 31 - 1, -2, -(2 ** 31)], np.int64), len(at)).astype(np.int32)


def _empty_state(rng, n_ops, L):
    return dict(kp_lm=np.zeros(0, np.int32), kp_outl=np.zeros(0, np.uint8), n_matches=int(rng.integers(0, 3)), L=L,
                op_view=rng.integers(-1, 3, n_ops).astype(np.int32), op_lm=rng.permutation(max(L, n_ops))[:n_ops].astype(np.int32))


def replay_draw(rng, i):
    seed = int(rng.integers(0, 1 << 30))
    n, n_ops = draw_size(rng, 3000), draw_size(rng, 3000)
    L = int(rng.choice([0, 4, max(1, draw_size(rng, 20000)), max(4, (n + n_ops) * 2 // 3), max(1, n // 2)]))
    dens = dict(p_held=float(rng.choice([0.0, 0.1, 0.5, 0.9, 1.0])), p_dup=float(rng.choice([0.0, 0.3, 0.8])), p_stale=float(rng.choice([0.0, 0.3, 1.0])))
    ops = dict(p_own=float(rng.choice([0.0, 0.33, 1.0])), p_skip=float(rng.choice([0.0, 0.05, 0.5])))
    lm = TC.replay_state(seed, n, n_ops, L or None, **dens, **ops) if n else _empty_state(rng, n_ops, L or 4)
    vw = RC.replay_state(seed, n, L or None, **dens, **ops) if n else _empty_state(rng, 0, L or 4)
    for s in (lm, vw):
        _invalid_ops(rng, s, n)
    return dict(lm=lm, vw=vw, caller=bool(rng.integers(0, 2)), orders=(rng.permutation(len(lm["op_view"])), rng.permutation(len(vw["op_view"]))),
                what=params(seed=seed, n=n, n_ops=n_ops, L=lm["L"], **dens, **ops))


def _replay_tags(s, want, valid_view, valid_lm):
    kp0, outl0 = s["kp_lm"], s["kp_outl"]
    out_kp, out_outl, nm = want
    n_valid = len(valid_view)
    tags = set()
    if nm > s["n_matches"]:
        tags.add("fresh insert")
    if n_valid > nm - s["n_matches"]:
        tags.add("replace")
    if ((kp0 >= 0) & (out_kp == -1)).any():
        tags.add("another view erased")
    if n_valid and (kp0[valid_view] == valid_lm).any():
        tags.add("op on its own holder")
    if n_valid and (np.bincount(kp0[kp0 >= 0], minlength=s["L"])[valid_lm] >= 2).any():
        tags.add("duplicated holder")
    if ((kp0 < 0) & (outl0 == 2) & (out_outl == 2) & (out_kp >= 0)).any():
        tags.add("stale flag kept")
    if n_valid < len(s["op_view"]):
        tags.add("skipped op")
    return tags


def replay_reference(c):
    """the batched twins of the exhaustive CPU proofs on the one state: seq_batch of test_track_ref.py (ops in ascending landmark index) and of
    test_refkf_ref.py (ascending view index)"""
    want, reached = {}, set()
    for which, s, mod in (("lm", c["lm"], LR), ("vw", c["vw"], VR)):
        n, L = len(s["kp_lm"]), s["L"]
        ok = (s["op_view"] >= 0) & (s["op_view"] < n) & (s["op_lm"] >= 0) & (s["op_lm"] < L)
        vv, vl = s["op_view"][ok].astype(np.int64), s["op_lm"][ok].astype(np.int64)
        dense = np.full((1, L if which == "lm" else n), -1, np.int64)
        if which == "lm":
            dense[0, vl] = vv                                      # opv[k] = the view landmark k's op targets
        else:
            dense[0, vv] = vl                                      # opl[v] = the landmark of view v's op
        if n:
            kp, outl, nm = mod.seq_batch(s["kp_lm"].astype(np.int64)[None, :], s["kp_outl"][None, :], np.array([s["n_matches"]], np.int64), dense)
            w = (kp[0], outl[0], int(nm[0]))
        else:                                                      # a frame without views: every op names a view outside it, nothing changes
            assert not ok.any()
            w = (s["kp_lm"], s["kp_outl"], s["n_matches"])
        for k, a in zip(REPLAY_OUT, w):
            want["%s.%s" % (which, k)] = a
        reached |= {"%s: %s" % (which, t) for t in _replay_tags(s, w, vv, vl)}
    return want, reached


def replay_device(ctx, c):
    from test_gpu_refkf import associate_views_device
    from test_gpu_track import associate_device
    st = ctx.stream(c["caller"])
    got = {}
    for which, f, order in (("lm", associate_device, c["orders"][0]), ("vw", associate_views_device, c["orders"][1])):
        for k, a in zip(REPLAY_OUT, f(ctx.tracker, c[which], order, stream=st)):
            got["%s.%s" % (which, k)] = a
    return got


# ---- the exhaustive spaces: B cases with disjoint view and landmark ranges are one state (case c: views [c*n, (c+1)*n), landmarks [c*L, (c+1)*L))
EXHAUSTIVE_SIZES = [(1, 1), (1, 4), (2, 2), (2, 4), (3, 3), (4, 2), (3, 4), (4, 3)]
CHUNK = 1 << 20


def concatenate(which, kp, fl, op, n, L, rng, n_matches=7):
    """-> the state dict of B concatenated cases, its ops in a shuffled array order.  which = "lm": op [B, L] holds views; "vw": op [B, n] landmarks"""
    B = len(kp)
    base_v, base_l = (np.arange(B, dtype=np.int64) * n)[:, None], (np.arange(B, dtype=np.int64) * L)[:, None]
    if which == "lm":
        op_view, op_lm = np.where(op >= 0, op + base_v, -1), np.broadcast_to(base_l + np.arange(L)[None, :], op.shape)
    else:
        op_view, op_lm = np.broadcast_to(base_v + np.arange(n)[None, :], op.shape), np.where(op >= 0, op + base_l, -1)
    p = rng.permutation(op.size)
    return dict(kp_lm=np.where(kp >= 0, kp + base_l, -1).astype(np.int32).reshape(-1), kp_outl=np.ascontiguousarray(fl, np.uint8).reshape(-1), n_matches=n_matches,
                L=B * L, op_view=op_view.reshape(-1)[p].astype(np.int32), op_lm=op_lm.reshape(-1)[p].astype(np.int32))


def split(got, B, n, L):
    """a concatenated result back into [B, n] cases with their own landmark numbers"""
    kp = got[0].astype(np.int64).reshape(B, n)
    return np.where(kp >= 0, kp - (np.arange(B, dtype=np.int64) * L)[:, None], -1), got[1].reshape(B, n), got[2]


def exhaustive_chunks(which, n, L, chunk=CHUNK, stride=1):
    """(first index, kp, flags, ops) over the full product of the module's state_tables, every stride-th case"""
    mod = LR if which == "lm" else VR
    kp, fl, op = mod.state_tables(n, L)
    total = len(kp) * len(fl) * len(op)
    for s in range(0, total, chunk * stride):
        idx = np.arange(s, min(s + chunk * stride, total), stride)
        yield s, kp[idx // (len(fl) * len(op))], fl[(idx // len(op)) % len(fl)], op[idx % len(op)]


def exhaustive_check(which, n, L, run, seed=0, chunk=CHUNK, stride=1):
    """every case of the n x L space through `run(state) -> (kp_lm, kp_outl, n_matches)` in chunks; -> (cases, first mismatch message or None)"""
    mod = LR if which == "lm" else VR
    rng = np.random.default_rng(seed)
    count = 0
    for s0, kp, fl, op in exhaustive_chunks(which, n, L, chunk, stride):
        B = len(kp)
        nm0 = np.zeros(B, np.int64)
        w_kp, w_fl, w_nm = mod.seq_batch(kp, fl, nm0, op)
        state = concatenate(which, kp, fl, op, n, L, rng)
        g_kp, g_fl, g_nm = split(run(state), B, n, L)
        for what, w, g in (("kp_lm", w_kp, g_kp), ("kp_outl", w_fl, g_fl)):
            bad = np.nonzero((w != g).any(1))[0]
            if len(bad):
                b = int(bad[0])
                return count, "replay %s exhaustive %d x %d: case %d %s differs: state %s flags %s ops %s want %s got %s" % (
                    which, n, L, s0 + b * stride, what, kp[b].tolist(), fl[b].tolist(), op[b].tolist(), w[b].tolist(), g[b].tolist())
        if g_nm != state["n_matches"] + int(w_nm.sum()):
            return count, "replay %s exhaustive %d x %d: chunk at %d: n_matches %d, want %d + %d" % (which, n, L, s0, g_nm, state["n_matches"], int(w_nm.sum()))
        count += B
    return count, None


def device_runner(ctx, which):
    from test_gpu_refkf import associate_views_device
    from test_gpu_track import associate_device
    f = associate_device if which == "lm" else associate_views_device
    return lambda state: f(ctx.tracker, state)


# ================================================================ frame_state: hs_frame_views_device, hs_track_discard_device
FRAME_STATE_TAGS = ["drop_bad on", "drop_bad off", "a bad landmark dropped", "mode motion", "mode local", "sensor 0", "sensor 1", "sensor 2", "HS_POSE_TOO_FEW",
                    "truncated edge count", "outlier removed", "outlier kept"]


def frame_state_draw(rng, i):
    n, L = max(1, draw_size(rng, 3000)), max(1, draw_size(rng, 20000))
    p_held, p_bad, p_out = float(rng.choice([0.0, 0.3, 0.7, 1.0])), float(rng.choice([0.0, 0.2, 1.0])), float(rng.choice([0.0, 0.3, 1.0]))
    kp_lm = np.where(rng.random(n) < p_held, rng.integers(0, L, n), -1).astype(np.int32)
    kp_outl = rng.integers(0, 3, n).astype(np.uint8)                  # also what the chain never makes: a held view without an entry, a flagged empty view
    lm_nobs, lm_bad = rng.integers(0, 4, L).astype(np.int32), (rng.random(L) < p_bad).astype(np.uint8)
    drop_bad, mode, sensor = int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(0, 3))
    status = int(rng.choice([0, 0, 1, 2]))                            # 1 = HS_POSE_TOO_FEW
    edges_kp = rng.permutation(np.nonzero((kp_lm >= 0) | (rng.random(n) < 0.1))[0])     # each view in at most one edge, some on views that hold nothing
    outlier = (rng.random(len(edges_kp)) < p_out).astype(np.uint8)
    cap = draw_cap(rng, len(edges_kp))
    n_edges = int(rng.choice([len(edges_kp), min(cap, len(edges_kp)), len(edges_kp) // 2]))
    nm = int(rng.integers(n, n + 5))
    return dict(kp_lm=kp_lm, kp_outl=kp_outl, lm_nobs=lm_nobs, lm_bad=lm_bad, drop_bad=drop_bad, mode=mode, sensor=sensor, status=status, edges_kp=edges_kp,
                outlier=outlier, cap=cap, n_edges=n_edges, nm=nm, caller=bool(rng.integers(0, 2)),
                what=params(n=n, L=L, p_held=p_held, p_bad=p_bad, p_out=p_out, drop_bad=drop_bad, mode=mode, sensor=sensor, status=status, edges=len(edges_kp), n_edges=n_edges,
                            cap=cap))


def frame_state_reference(c):
    """the numpy models of tests/test_gpu_track.py: the views after frame_views feed the discard"""
    from test_gpu_track import _discard_numpy, _frame_views_numpy
    v = _frame_views_numpy(c["kp_lm"], c["kp_outl"], c["nm"], c["lm_bad"], c["lm_nobs"], c["drop_bad"])
    ne = min(c["n_edges"], c["cap"])
    d = _discard_numpy(c["mode"], c["sensor"], c["edges_kp"], ne, c["outlier"], c["status"] != 1, v[0].astype(np.int32), v[1].astype(np.uint8), v[2], c["lm_nobs"])
    want = dict(zip(("views.kp_lm", "views.kp_outl", "views.n_matches", "views.kp_lm_obs"), v))
    want.update(zip(("discard.kp_lm", "discard.kp_outl", "discard.n_matches", "discard.count"), d))
    removed, kept = (v[0] >= 0) & (d[0] < 0), (d[0] >= 0) & (d[1] == 2)
    reached = {"drop_bad on" if c["drop_bad"] else "drop_bad off", "mode local" if c["mode"] else "mode motion", "sensor %d" % c["sensor"]}
    reached |= {t for t, hit in (("a bad landmark dropped", v[2] < c["nm"]), ("HS_POSE_TOO_FEW", c["status"] == 1), ("truncated edge count", c["n_edges"] > c["cap"]),
                                 ("outlier removed", removed.any()), ("outlier kept", kept[c["edges_kp"][:ne]].any())) if hit}
    return want, reached


def frame_state_device(ctx, c):
    from test_gpu_track import discard_device, frame_views_device
    st = ctx.stream(c["caller"])
    v = frame_views_device(ctx.tracker, c["kp_lm"], c["kp_outl"], c["nm"], c["lm_bad"], c["lm_nobs"], c["drop_bad"], stream=st)
    d = discard_device(ctx.tracker, c["mode"], c["sensor"], c["edges_kp"], c["n_edges"], c["cap"], c["outlier"], c["status"], v[0], v[1], v[2], c["lm_nobs"], stream=st)
    got = dict(zip(("views.kp_lm", "views.kp_outl", "views.n_matches", "views.kp_lm_obs"), v))
    got.update(zip(("discard.kp_lm", "discard.kp_outl", "discard.n_matches", "discard.count"), d))
    return got


# ================================================================ kf_votes: hs_kf_votes(_device)
VOTES_TAGS = ["LDS counters", "global counters", "empty counter", "single (nmax, pKFmax) fallback", "list <= HS_KF_SORT_PASS", "list > HS_KF_SORT_PASS", "n_ordered > cap",
              "tie for the maximum", "tie inside the list", "self excluded by id", "bad key frame counted but not chosen"]


def votes_draw(rng, i):
    seed = int(rng.integers(0, 1 << 30))
    kind = rng.choice(["plain", "plain", "plain", "long", "global"]) if i % 8 else ("global", "long")[(i // 8) % 2]
    if kind == "global":                                              # the one shape beyond the LDS limit: Q <= 2, tiny lists
        n_kf, L, max_obs, big, Q, window = HS_KF_LDS_SLOTS + 1, 60, 30, [(0, 500)], int(rng.integers(1, 3)), True
    elif kind == "long":                                              # a list beyond one sort pass: one landmark seen by more than HS_KF_SORT_PASS key frames
        n_kf = int(rng.integers(HS_KF_SORT_PASS + 2, 2000))
        L, max_obs, big, Q, window = draw_size(rng, 300, 1), 8, [(0, int(rng.integers(HS_KF_SORT_PASS + 1, n_kf + 1)))], int(rng.integers(1, 3)), True
    else:
        n_kf, L = max(1, draw_size(rng, 1100)), draw_size(rng, 3000)
        max_obs, big, Q, window = int(rng.choice([1, 3, 12, 40])), [], int(rng.choice([0, 1, 2, 5])), bool(rng.integers(0, 2)) or n_kf > 300
    p_bad_lm, p_bad_kf = float(rng.choice([0.0, 0.05, 0.5])), float(rng.choice([0.0, 0.05, 0.5]))
    T = KC.random_table(seed, n_kf, L, max_obs=max_obs, big=[b for b in big if b[0] < L], window=window, p_bad_lm=p_bad_lm, p_bad_kf=p_bad_kf)
    queries = []
    for q in range(Q):
        m = min(draw_size(rng, 2000), 60 if kind == "global" else 2000) if L else 0
        lms = rng.integers(0, L, m) if m else np.zeros(0, np.int64)
        if m and kind != "plain" and rng.random() < 0.8:
            lms[0] = 0                                                # the big landmark votes
        if m > 1 and rng.random() < 0.3:
            lms[m // 2:] = lms[:m - m // 2]                           # landmarks listed twice count twice
        queries.append(lms)
    off, q_lm = KC.csr(queries)
    ids = None
    if Q and rng.random() < 0.6:
        ids = np.where(rng.random(Q) < 0.7, T["kf_id"][rng.integers(0, n_kf, Q)], -1).astype(np.int64)
    count_bad_kf, th = int(rng.integers(0, 2)), int(rng.choice([1, 1, 2, 5, 15]))
    full = RK.votes_fast(T, off, q_lm, ids, count_bad_kf, th, 0)
    cap = draw_cap(rng, int(full["n_ordered"][int(rng.integers(0, Q))]) if Q else 3)
    device = bool(rng.integers(0, 2)) or kind == "global"
    weights = bool(rng.integers(0, 4)) or n_kf > HS_KF_LDS_SLOTS      # beyond the LDS limit the rows are the counters: required
    return dict(T=T, off=off, q_lm=q_lm, ids=ids, count_bad_kf=count_bad_kf, th=th, cap=cap, device=device, weights=weights, caller=bool(rng.integers(0, 2)),
                what=params(seed=seed, kind=kind, n_kf=n_kf, L=L, max_obs=max_obs, window=window, p_bad_lm=p_bad_lm, p_bad_kf=p_bad_kf, Q=Q, items=len(q_lm),
                            self_id=ids is not None, count_bad_kf=count_bad_kf, th=th, cap=cap, form="device" if device else "host", weights=weights))


def votes_reference(c):
    T, cap = c["T"], c["cap"]
    w = RK.votes_fast(T, c["off"], c["q_lm"], c["ids"], c["count_bad_kf"], c["th"], cap)
    want = {k: w[k] for k in RK.VOTE_KEYS if k != "weights" or c["weights"]}
    n_kf, Q = len(T["kf_id"]), len(c["off"]) - 1
    reached = {"LDS counters" if n_kf <= HS_KF_LDS_SLOTS else "global counters"} if Q else set()
    bad_kf = T["kf_bad"] != 0
    for q in range(Q):
        row, ordered = w["weights"][q], w["ordered"][q]
        elig = (row > 0) & ~(bad_kf if c["count_bad_kf"] else np.zeros(n_kf, bool))
        if w["max_slot"][q] < 0:
            reached.add("empty counter")
        elif not (elig & (row >= c["th"])).any():
            reached.add("single (nmax, pKFmax) fallback")
        if ordered:
            reached.add("list <= HS_KF_SORT_PASS" if len(ordered) <= HS_KF_SORT_PASS else "list > HS_KF_SORT_PASS")
        if len(ordered) > cap:
            reached.add("n_ordered > cap")
        if elig.any() and int((elig & (row == w["max_count"][q])).sum()) >= 2:
            reached.add("tie for the maximum")
        if any(a[1] == b[1] for a, b in zip(ordered, ordered[1:])):
            reached.add("tie inside the list")
        if c["count_bad_kf"] and (bad_kf & (row > 0)).any():
            reached.add("bad key frame counted but not chosen")
        if c["ids"] is not None and c["ids"][q] != -1:
            lms = c["q_lm"][int(c["off"][q]):int(c["off"][q + 1])].astype(np.int64)
            lms = lms[T["lm_bad"][lms] == 0]
            _, idx = RK._expand(T, lms)
            if (T["kf_id"][T["lm_obs_kf"][idx]] == c["ids"][q]).any():
                reached.add("self excluded by id")
    return want, reached


def votes_device(ctx, c):
    import ctypes as C
    from devbuf import dev, out_buf, read
    from hyslam_amd import _native as N
    from test_gpu_kfgraph import c_votes, native_table
    T, cap = c["T"], c["cap"]
    Q, n_kf = len(c["off"]) - 1, len(T["kf_id"])
    if not c["device"]:
        st, out = c_votes(ctx.matcher, T, c["off"], c["q_lm"], c["ids"], c["count_bad_kf"], c["th"], cap, weights=c["weights"], fill=0x55)
        assert st == N.HS_OK, st
        return {k: v for k, v in out.items() if v is not None}
    ex, s = ctx.ex, ctx.stream(c["caller"])
    KT, keep = native_table(N, T, dev=True)
    ins = [dev(np.ascontiguousarray(c["off"], np.int64)), dev(np.ascontiguousarray(c["q_lm"], np.int32)), None if c["ids"] is None else dev(c["ids"])]
    shapes = dict(weights=(Q, n_kf), max_slot=(Q,), max_count=(Q,), ordered_slot=(Q, cap), ordered_weight=(Q, cap), n_ordered=(Q,))
    outs = {k: out_buf(4 * int(np.prod(shapes[k]))) for k in RK.VOTE_KEYS if k != "weights" or c["weights"]}
    ptr = lambda k: outs[k].ptr if k in outs else None
    N.check(ex._h, ex._lib.hs_kf_votes_device(ex._h, C.byref(KT), Q, ins[0].ptr, ins[1].ptr, ins[2].ptr if ins[2] else None, c["count_bad_kf"], c["th"], ptr("weights"),
                                              ptr("max_slot"), ptr("max_count"), ptr("ordered_slot"), ptr("ordered_weight"), cap, ptr("n_ordered"), s.ptr or None))
    s.synchronize()
    return {k: read(b, np.int32, int(np.prod(shapes[k]))).reshape(shapes[k]) for k, b in outs.items()}


# ================================================================ kf_redundancy: hs_kf_redundancy(_device)
RED_TAGS = ["mono", "depth gate passed", "depth gate refused", "Observations() == th_obs", "octave gate at +1", "verdict exactly on frac * n_mps", "empty candidate"]


def red_draw(rng, i):
    seed = int(rng.integers(0, 1 << 30))
    n_kf, L = max(1, draw_size(rng, 1100)), max(1, draw_size(rng, 3000))
    max_obs, window = int(rng.choice([1, 4, 12, 40])), bool(rng.integers(0, 2)) or n_kf > 300
    p_bad_lm = float(rng.choice([0.0, 0.05, 0.5]))
    T = KC.random_table(seed, n_kf, L, max_obs=max_obs, window=window, p_bad_lm=p_bad_lm)
    sizes = [draw_size(rng, 2000) for _ in range(int(rng.choice([0, 1, 3, 7])))]
    cand = KC.random_candidates(seed + 1, T, sizes)
    is_mono, th_obs = int(rng.integers(0, 2)), int(rng.choice([1, 2, 3, 3, 5]))
    frac = float(np.float32(rng.choice([0.9, 0.5, 0.05, 0.75])))
    first = RK.redundancy_fast(T, cand["cand_slot"], cand["cand_th_depth"], cand["cand_offsets"], cand["item_lm"], cand["item_octave"], cand["item_depth"], is_mono, th_obs, frac)
    live = np.nonzero(first["n_mps"] > 0)[0]
    if len(live) and rng.random() < 0.5:                              # a fraction that puts one candidate's verdict exactly on the product, where float allows it
        c = int(live[int(rng.integers(0, len(live)))])
        frac = float(np.float32(first["n_redundant"][c]) / np.float32(first["n_mps"][c]))
    return dict(T=T, cand=cand, is_mono=is_mono, th_obs=th_obs, frac=frac, device=bool(rng.integers(0, 2)), caller=bool(rng.integers(0, 2)),
                what=params(seed=seed, n_kf=n_kf, L=L, max_obs=max_obs, window=window, p_bad_lm=p_bad_lm, sizes=sizes, is_mono=is_mono, th_obs=th_obs, frac=repr(frac)))


def red_reference(c):
    T, cd = c["T"], c["cand"]
    w = RK.redundancy_fast(T, cd["cand_slot"], cd["cand_th_depth"], cd["cand_offsets"], cd["item_lm"], cd["item_octave"], cd["item_depth"], c["is_mono"], c["th_obs"], c["frac"])
    want = {k: w[k] for k in RK.RED_KEYS}
    C = len(cd["cand_slot"])
    reached = {"mono"} if c["is_mono"] and C else set()
    for k in range(C):
        b, e = int(cd["cand_offsets"][k]), int(cd["cand_offsets"][k + 1])
        if b == e:
            reached.add("empty candidate")
        lm, level, depth = cd["item_lm"][b:e].astype(np.int64), cd["item_octave"][b:e].astype(np.int64), cd["item_depth"][b:e]
        keep = T["lm_bad"][lm] == 0
        if not c["is_mono"]:
            gate = (depth > np.float32(cd["cand_th_depth"][k])) | (depth < 0)
            reached |= {t for t, hit in (("depth gate refused", (keep & gate).any()), ("depth gate passed", (keep & ~gate).any())) if hit}
            keep &= ~gate
        if (T["lm_nobs"][lm[keep]] == c["th_obs"]).any():
            reached.add("Observations() == th_obs")
        use = keep & (T["lm_nobs"][lm] > c["th_obs"])
        owner, idx = RK._expand(T, lm[use])
        if ((T["lm_obs_kf"][idx] != cd["cand_slot"][k]) & (T["lm_obs_octave"][idx] == level[use][owner] + 1)).any():
            reached.add("octave gate at +1")
        if w["n_mps"][k] > 0 and np.float32(w["n_redundant"][k]) == np.float32(c["frac"]) * np.float32(w["n_mps"][k]):
            reached.add("verdict exactly on frac * n_mps")
    return want, reached


def red_device(ctx, c):
    import ctypes as C
    from devbuf import dev, out_buf, read
    from hyslam_amd import _native as N
    from test_gpu_kfgraph import native_table
    T, cd = c["T"], c["cand"]
    if not c["device"]:
        got = ctx.matcher.KeyFrameRedundancy(T, cd["cand_slot"], cd["cand_th_depth"], cand_offsets=cd["cand_offsets"], item_lm=cd["item_lm"], item_octave=cd["item_octave"],
                                             item_depth=cd["item_depth"], is_mono=c["is_mono"], th_obs=c["th_obs"], frac_redundant=c["frac"])
        return {k: got[k] for k in RK.RED_KEYS}
    ex, s, Cn = ctx.ex, ctx.stream(c["caller"]), len(cd["cand_slot"])
    KT, keep = native_table(N, T, dev=True)
    cin = [dev(cd[k]) for k in ("cand_slot", "cand_th_depth", "cand_offsets", "item_lm", "item_octave", "item_depth")]
    outs = out_buf(4 * Cn), out_buf(4 * Cn), out_buf(Cn)
    N.check(ex._h, ex._lib.hs_kf_redundancy_device(ex._h, C.byref(KT), Cn, *[b.ptr for b in cin], c["is_mono"], c["th_obs"], c["frac"], *[o.ptr for o in outs], s.ptr or None))
    s.synchronize()
    return dict(n_mps=read(outs[0], np.int32, Cn), n_redundant=read(outs[1], np.int32, Cn), cull=read(outs[2], np.uint8, Cn))


# ================================================================ landmark_descriptors: hs_landmark_best_descriptors(_device)
DESC_TAGS = ["n = 0", "n = 1", "n = 2", "wave path", "workgroup path", "tie for the median", "tie for the minimum"]


def desc_draw(rng, i):
    from test_gpu_landmark_descriptors import csr, ragged_batch
    seed = int(rng.integers(0, 1 << 30))
    L, n_max = draw_size(rng, 400), int(rng.choice([2, 8, 40, 63, 64, 65, 90]))
    big = [(int(rng.integers(0, L)), max(LM_SMALL + 1, draw_size(rng, 1300))) for _ in range(int(rng.integers(0, 3)))] if L else []
    lms = ragged_batch(seed, L, big=big, n_max=max(2, n_max))
    for j in rng.integers(0, max(L, 1), int(rng.integers(0, 4)) if L else 0):      # sizes the generator draws rarely
        lms[j] = lms[j][:int(rng.integers(0, 3))]
    off, desc = csr(lms)
    lead = int(rng.choice([0, 0, 1, 13]))                                          # offsets need not start at 0: leading descriptors nobody owns
    if lead:
        off, desc = off + lead, np.concatenate([rng.integers(0, 256, (lead, 32), dtype=np.uint8), desc])
    return dict(lms=lms, off=off, desc=desc, device=bool(rng.integers(0, 2)), caller=bool(rng.integers(0, 2)),
                what=params(seed=seed, L=L, n_max=n_max, big=big, lead=lead))


def _median_rows(d):
    """the sorted distance rows of one landmark and the median index (ref_landmark's matrix, kept for the tags)"""
    pop = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)
    D = np.zeros((len(d), len(d)), np.int32)
    for b in range(32):
        D += pop[d[:, b][:, None] ^ d[:, b][None, :]]
    return np.sort(D, axis=1), int(0.5 * (len(d) - 1))


def desc_reference(c):
    best, med = RL.distinctive_descriptors_fast(c["lms"])
    reached = set()
    for d in c["lms"]:
        n = len(d)
        reached |= {"n = %d" % n} if n <= 2 else set()
        if n:
            reached.add("wave path" if n <= LM_SMALL else "workgroup path")
        if n >= 2:
            rows, k = _median_rows(np.asarray(d, np.uint8))
            m = rows[:, k]
            if (rows[:, k + 1] == m).any() or (k and (rows[:, k - 1] == m).any()):
                reached.add("tie for the median")                                   # the k-th smallest of a row is not alone in it
            if int((m == m.min()).sum()) >= 2:
                reached.add("tie for the minimum")                                  # several rows share the best median: the first one wins
    return dict(best=best, median=med), reached


def desc_device(ctx, c):
    from devbuf import dev, out_buf, read
    L = len(c["lms"])
    if not c["device"]:
        b, m = ctx.matcher.ComputeDistinctiveDescriptors(offsets=c["off"], desc=c["desc"])
        return dict(best=b, median=m)
    s = ctx.stream(c["caller"])
    d_off, d_desc, d_b, d_m = dev(c["off"]), dev(c["desc"]), out_buf(4 * L), out_buf(4 * L)
    ctx.ex.landmark_best_descriptors_device(d_off.ptr, L, d_desc.ptr, d_b.ptr, d_m.ptr, stream=s.ptr)
    s.synchronize()
    return dict(best=read(d_b, np.int32, L), median=read(d_m, np.int32, L))


# ================================================================ landmark_entries: hs_landmark_update_entries(_device)
ENTRY_TAGS = ["0 observations", "1 observation", ">= 2 observations", "camera centre on the point", "keypoint without association", "keypoint of another landmark",
              "keypoint size 0", "keypoint size 3e30", "camera centre z = -0", "camera centre near the origin", "landmark z = -0"]
ENTRY_KEYS = ("normal", "min_dist", "max_dist", "mean_dist", "size", "best", "median", "flags")
LMS_REST = ("pos", "assoc_kp", "prev_angle", "skip")


def entries_draw(rng, i):
    seed = int(rng.integers(0, 1 << 30))
    L, n_max = draw_size(rng, 600), int(rng.choice([0, 1, 2, 40, 63, 64, 65, 130]))
    big = [(int(rng.integers(0, L)), draw_size(rng, 1300)) for _ in range(int(rng.integers(0, 3)))] if L else []
    special, rate, p_empty = bool(rng.integers(0, 4)), float(rng.choice([1.0, 5.0, 20.0])), float(rng.choice([0.0, 0.03, 0.5]))
    ent, off, ob, descs = LE.random_batch(seed, L, n_max=n_max, big=big, special=special, rate=rate, p_empty=p_empty)
    factors = (2.0, 0.5) if rng.random() < 0.7 else (float(np.float32(rng.uniform(1.1, 3))), float(np.float32(rng.uniform(0.1, 0.9))))
    device = bool(rng.integers(0, 2))
    c = dict(ent=ent, off=off, ob=ob, descs=descs, factors=factors, device=device, caller=bool(rng.integers(0, 2)), scatter=device and bool(rng.integers(0, 2)))
    if c["scatter"]:                                                  # a permuted index map, some -1, some past the end (skipped); the valid ones distinct
        n_lms = L + int(rng.integers(0, 40))
        c["lms"] = np.frombuffer(rng.integers(0, 256, n_lms * TC.LM_DTYPE.itemsize, dtype=np.uint8).tobytes(), TC.LM_DTYPE).copy()
        index = rng.permutation(n_lms)[:L].astype(np.int32)
        out = rng.random(L) < 0.1
        index[out] = rng.choice(np.array([-1, -7, n_lms, n_lms + 5, 2 ** 31 - 1], np.int64), int(out.sum())).astype(np.int32)
        c["index"] = index
    c["what"] = params(seed=seed, L=L, n_max=n_max, big=big, special=special, rate=rate, p_empty=p_empty, factors=factors, form="device" if device else "host",
                       scatter=c["scatter"])
    return c


def entries_reference(c):
    ent, off, ob, descs = c["ent"], c["off"], c["ob"], c["descs"]
    w = RE.update_entries_fast(ent, off, ob, descs, max_factor=c["factors"][0], min_factor=c["factors"][1])
    want = {k: w[k] for k in ENTRY_KEYS}
    if c["scatter"]:
        exp, n_lms = c["lms"].copy(), len(c["lms"])
        for i in np.nonzero((c["index"] >= 0) & (c["index"] < n_lms))[0]:
            t = c["index"][i]
            if w["flags"][i] & RE.HS_LM_SET_NORMAL_DEPTH:
                exp["normal"][t], exp["min_dist"][t], exp["max_dist"][t] = w["normal"][i], w["min_dist"][i], w["max_dist"][i]
            exp["size"][t] = w["size"][i]
            if w["best"][i] >= 0:
                exp["desc"][t] = descs[i][w["best"][i]]
        want.update(_lms_fields(exp))
    cnt = np.diff(off)
    owner = np.repeat(np.arange(len(ent)), cnt)
    reached = {t for t, hit in (("0 observations", (cnt == 0).any()), ("1 observation", (cnt == 1).any()), (">= 2 observations", (cnt >= 2).any()),
                                ("landmark z = -0", (np.signbit(ent["pos"][:, 2]) & (ent["pos"][:, 2] == 0)).any())) if hit}
    if len(ob):
        pos = ent["pos"][owner]
        reached |= {t for t, hit in (("camera centre on the point", (ob["Ow"] == pos).all(1).any()), ("keypoint without association", (ob["assoc"] == 0).any()),
                                     ("keypoint of another landmark", (ob["assoc_pos"] != pos).any()), ("keypoint size 0", (ob["kp_size"] == 0).any()),
                                     ("keypoint size 3e30", (ob["kp_size"] == np.float32(3e30)).any()),
                                     ("camera centre z = -0", (np.signbit(ob["Ow"][:, 2]) & (ob["Ow"][:, 2] == 0)).any()),
                                     ("camera centre near the origin", (np.abs(ob["Ow"]).max(1) < 0.01).any())) if hit}
    return want, reached


def _lms_fields(lms):
    """the records as the arrays the comparison names: the four fields the scatter writes, and everything it must leave alone"""
    out = {"lms." + f: np.ascontiguousarray(lms[f]) for f in ("normal", "min_dist", "max_dist", "size", "desc")}
    out["lms.untouched"] = np.concatenate([np.ascontiguousarray(lms[f]).reshape(len(lms), -1).view(np.uint8) for f in LMS_REST], 1) if len(lms) else np.zeros((0, 24), np.uint8)
    return out


def entries_device(ctx, c):
    from devbuf import dev, out_buf, read
    from test_gpu_landmark_entries import desc_csr
    ent, off, ob, descs = c["ent"], c["off"], c["ob"], c["descs"]
    L = len(ent)
    if not c["device"]:
        got = ctx.matcher.UpdateLandmarkEntries(ent, obs_offsets=off, obs=ob, descriptors=descs, max_dist_factor=c["factors"][0], min_dist_factor=c["factors"][1])
        return {k: got[k] for k in ENTRY_KEYS}
    from hyslam_amd import _native as N
    s = ctx.stream(c["caller"])
    doff, dflat = desc_csr(descs)
    ins = [dev(a) for a in (ent, off, ob, doff, dflat)]
    outs = [out_buf(L * 12)] + [out_buf(L * 4) for _ in range(7)]
    kw = {}
    if c["scatter"]:
        d_lms, d_idx = dev(c["lms"]), dev(c["index"])
        kw = dict(d_lms=d_lms.ptr, d_lm_index=d_idx.ptr, n_lms=len(c["lms"]))
    ctx.ex.landmark_update_entries_device(L, *[b.ptr for b in ins], *[o.ptr for o in outs], params=N.LmEntryParams(*c["factors"]), stream=s.ptr, **kw)
    s.synchronize()
    got = {k: read(o, np.float32 if j < 5 else np.int32, L * (3 if j == 0 else 1)) for j, (k, o) in enumerate(zip(ENTRY_KEYS, outs))}
    got["normal"] = got["normal"].reshape(L, 3)
    empty = np.diff(off) == 0
    for k in ("normal", "min_dist", "max_dist", "mean_dist"):         # N = 0 leaves the output alone: the fill pattern still there reads as "not set" (NaN)
        rows = got[k][empty]
        rows[rows.view(np.uint32) == 0x55555555] = np.nan
        got[k][empty] = rows
    if c["scatter"]:
        got.update(_lms_fields(d_lms.to_numpy(TC.LM_DTYPE, len(c["lms"]))))
    return got


# ================================================================ local_map: hs_local_keyframes(_device), hs_local_points(_device), hs_landmark_gather_device
LOCAL_TAGS = ["n_max reached", "neighbour added", "parent added", "bad key frame voted", "no votes", "points cap truncates", "frame associations removed",
              "held landmark left out", "gather index outside the array", "gather n_sel > cap"]


def _walk_tags(c):
    """UpdateLocalKeyFrames once more, for the tags alone: which of its ways out the walk took"""
    w, bad, neigh, parent = c["weights"], c["kf_bad"] != 0, c["neigh"], c["parent"]
    tags = {t for t, hit in (("bad key frame voted", ((w > 0) & bad).any()), ("no votes", not (w > 0).any())) if hit}
    local = set(np.nonzero((w > 0) & ~bad)[0].tolist())
    cur = -1
    while True:
        later = [x for x in local if x > cur]
        if not later:
            break
        cur = min(later)
        if RLM._exceeds(len(local), c["n_max"]):
            tags.add("n_max reached")
            break
        good = [int(x) for x in neigh[cur, :c["n_neighbor"]] if x >= 0 and not bad[x]]
        if good and good[0] not in local:
            tags.add("neighbour added")
        local |= set(good[:1])
        if parent[cur] >= 0:
            if int(parent[cur]) not in local:
                tags.add("parent added")
            break
    return tags


def local_draw(rng, i):
    seed = int(rng.integers(0, 1 << 30))
    n_kf, neigh_cap = max(1, draw_size(rng, 700)), int(rng.choice([1, 3, 10, 70]))
    pk = dict(p_vote=float(rng.choice([0.0, 0.02, 0.2, 0.9])), p_bad=float(rng.choice([0.0, 0.1, 0.6])), p_parent=float(rng.choice([0.0, 0.03, 0.5])))
    kf = LC.random_keyframes(seed, n_kf, neigh_cap=neigh_cap, **pk)
    L, max_obs, n_assoc, p_local = draw_size(rng, 5000), int(rng.choice([1, 4, 12])), draw_size(rng, 1500), float(rng.choice([0.0, 0.05, 0.3, 1.0]))
    big = [(int(rng.integers(0, L)), int(rng.integers(60, 400)))] if L and rng.random() < 0.4 else []
    T, local, flm = LC.random_points(seed, n_kf, L, max_obs=max_obs, big=big, n_assoc=n_assoc, p_local=p_local)
    dev_kf, dev_pts = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    if dev_pts and rng.random() < 0.4:                                # the device form skips a slot or an association outside the table (the host form refuses them)
        T["lm_obs_kf"] = T["lm_obs_kf"].copy()
        out = rng.random(len(T["lm_obs_kf"])) < 0.05
        T["lm_obs_kf"][out] = rng.choice(np.array([n_kf, n_kf + 64, -2], np.int64), int(out.sum())).astype(np.int32)
        out = rng.random(n_assoc) < 0.05
        flm[out] = rng.choice(np.array([L, L + 1024, -9], np.int64), int(out.sum())).astype(np.int32)
    n_sel = RLM.local_points_fast(T, local, flm, 0)["n_sel"]
    cap = draw_cap(rng, n_sel)
    lms = np.frombuffer(rng.integers(0, 256, L * TC.LM_DTYPE.itemsize, dtype=np.uint8).tobytes(), TC.LM_DTYPE).copy()
    sel = RLM.local_points_fast(T, local, flm, cap)["sel"].copy()    # the gather's input: the selection, a few entries replaced by indices outside [0, L)
    out = rng.random(cap) < (0.05 if rng.random() < 0.5 else 0.0)
    sel[out] = rng.choice(np.array([L, L + 7, -1, -5], np.int64), int(out.sum())).astype(np.int32)
    g_n = int(rng.choice([n_sel, min(n_sel, cap), cap + 3]))          # *d_n_sel: the full count, which may exceed cap
    return dict(kf=kf, T=T, local=local, flm=flm, cap=cap, lms=lms, g_sel=sel, g_n=g_n, dev_kf=dev_kf, dev_pts=dev_pts, caller=bool(rng.integers(0, 2)),
                what=params(seed=seed, n_kf=n_kf, neigh_cap=neigh_cap, **pk, n_max=kf["n_max"], n_neighbor=kf["n_neighbor"], L=L, max_obs=max_obs, big=big,
                            n_assoc=n_assoc, p_local=p_local, cap=cap, g_n=g_n, keyframes="device" if dev_kf else "host", points="device" if dev_pts else "host"))


def local_reference(c):
    kf, L = c["kf"], len(c["lms"])
    local, n_local = RLM.local_keyframes_fast(kf["weights"], kf["kf_bad"], kf["neigh"], kf["parent"], kf["n_max"], kf["n_neighbor"])
    pts = RLM.local_points_fast(c["T"], c["local"], c["flm"], c["cap"])
    sel, cap, n = c["g_sel"], c["cap"], min(c["g_n"], c["cap"])
    inside = (sel >= 0) & (sel < L)
    rec = RLM.gather(c["lms"], np.where(inside, sel, 0), n, cap) if L else np.zeros(cap, TC.LM_DTYPE)
    hole = ~inside & (np.arange(cap) < n)
    rec[hole] = np.zeros(1, TC.LM_DTYPE)
    rec["assoc_kp"], rec["skip"][hole] = -1, 1
    if not L:
        rec["skip"] = 1
    want = {"keyframes.local": local, "keyframes.n_local": n_local, "points.frame_remove": pts["frame_remove"], "points.sel": pts["sel"], "points.n_sel": pts["n_sel"],
            "gather.records": rec.view(np.uint8).reshape(cap, 80)}
    flm = c["flm"].astype(np.int64)
    ok = (flm >= 0) & (flm < len(c["T"]["lm_bad"]))
    reached = _walk_tags(kf) | {t for t, hit in (("points cap truncates", pts["n_sel"] > cap), ("frame associations removed", pts["frame_remove"].any()),
                                                 ("held landmark left out", ok.any() and (c["T"]["lm_bad"][flm[ok]] == 0).any() and pts["n_sel"] > 0),
                                                 ("gather index outside the array", hole.any()), ("gather n_sel > cap", c["g_n"] > cap)) if hit}
    return want, reached


def local_device(ctx, c):
    from devbuf import dev, out_buf, read
    from test_gpu_localmap import keyframes_device, points_device
    kf, s, cap = c["kf"], ctx.stream(c["caller"]), c["cap"]
    if c["dev_kf"]:
        local, n_local = keyframes_device(ctx.ex, kf, s)
    else:
        local, n_local = ctx.matcher.LocalKeyFrames(kf["weights"], kf["kf_bad"], kf["neigh"], kf["parent"], kf["n_max"], kf["n_neighbor"])
    if c["dev_pts"]:
        pts = points_device(ctx.ex, c["T"], c["local"], c["flm"], cap, s)
    else:
        pts = dict(zip(("frame_remove", "sel", "n_sel"), ctx.matcher.LocalPoints(c["T"], c["local"], c["flm"], cap=cap)))
    d_lms, d_sel, d_n, d_out = dev(c["lms"]), dev(c["g_sel"]), dev(np.array([c["g_n"]], np.int32)), out_buf(cap * 80)
    ctx.ex.landmark_gather_device(d_lms.ptr, len(c["lms"]), d_sel.ptr, d_n.ptr, cap, d_out.ptr, s.ptr)
    s.synchronize()
    return {"keyframes.local": local, "keyframes.n_local": n_local, "points.frame_remove": pts["frame_remove"], "points.sel": pts["sel"], "points.n_sel": pts["n_sel"],
            "gather.records": read(d_out, np.uint8, cap * 80).reshape(cap, 80)}


# ================================================================ place: one hs_place_db through a random sequence of add, add_device, erase, clear and queries
PLACE_TAGS = ["replace", "dedupe", "excluded", "d9", "tombstone", "query right after the slot-array regrow", "query after clear", "cap below the candidates",
              "no candidate"]
PLACE_REGROW = 1025                                                   # the slot arrays start with room for 1024 key frames and double


def place_draw(rng, i):
    seed = int(rng.integers(0, 1 << 30))
    regrow = i % 6 == 0                                               # the one long sequence: the 1 025th slot, and a query right behind it
    n_kf = int(rng.integers(PLACE_REGROW + 1, PLACE_REGROW + 40)) if regrow else max(1, draw_size(rng, 400))
    n_words = int(rng.choice([300, 1000, 100000]))
    lens = (5, 30) if regrow else [(5, 60), (1, 8), (20, 200)][int(rng.integers(0, 3))]
    big = [(int(rng.integers(0, n_kf)), int(rng.choice([1, 63, 64, 65, 129, 300])))] if rng.random() < 0.5 else []
    erase = float(rng.choice([0.0, 0.03, 0.3]))
    sc = PL.random_scene(seed, n_kf, n_words, lens, big, n_queries=int(rng.integers(2, 9)), erase=erase)
    p_query, p_erase, p_dev = (0.01 if regrow else float(rng.choice([0.02, 0.1]))), float(rng.choice([0.0, 0.02, 0.1])), float(rng.choice([0.0, 0.5, 1.0]))
    clear_at = int(rng.integers(0, n_kf)) if rng.random() < 0.4 and not regrow else -1
    ops, ref, slots, after_clear = [], RP.PlaceRecognizerRef(n_words), 0, False

    def query(tag=None):
        q = sc["queries"][int(rng.integers(0, len(sc["queries"])))]
        keys, _ = (ref.detect_reloc(q["query"][0], q["query"][1], sc["neigh"]) if q["mode"] == "reloc" else
                   ref.detect_loop(q["query"][0], q["query"][1], q["connected"], q["min_score"], sc["neigh"]))
        ops.append(("query", q, bool(rng.integers(0, 2)), draw_cap(rng, len(keys)), bool(rng.integers(0, 2)), tag))

    for j, (key, w, v) in enumerate(sc["entries"]):
        if j == clear_at:
            ops.append(("clear",))
            ref.clear()
            slots = 0
            query("query after clear")                                # on the empty database
            after_clear = True
        ops.append(("add", key, w, v, rng.random() < p_dev, int(rng.choice([0, 0, 3])), bool(rng.integers(0, 2))))
        ref.add(key, w, v)
        slots += 1
        if slots == PLACE_REGROW:
            query("query right after the slot-array regrow")
        elif rng.random() < p_query:
            query("query after clear" if after_clear else None)
        if rng.random() < p_erase and len(ref.bow) > 1:
            gone = list(ref.bow)[int(rng.integers(0, len(ref.bow)))]
            ops.append(("erase", gone))
            ref.erase(gone)
    for key in sc["erased"]:
        if key in ref.bow:
            ops.append(("erase", key))
            ref.erase(key)
    for _ in range(len(sc["queries"])):
        query("query after clear" if after_clear else None)
    return dict(ops=ops, neigh=sc["neigh"], n_words=n_words, caller=bool(rng.integers(0, 2)),
                what=params(seed=seed, n_kf=n_kf, n_words=n_words, lens=lens, big=big, erase=erase, p_query=p_query, p_erase=p_erase, p_dev=p_dev, clear_at=clear_at,
                            ops=len(ops)))


PLACE_OUT = ("n_cand", "cand", "words", "score", "acc", "best", "size")


def _place_pack(rows, live, slots):
    out = {k: np.concatenate([r[k] for r in rows]) if rows else np.zeros(0, np.float32 if k in ("score", "acc") else np.int32) for k in PLACE_OUT[1:6]}
    out["n_cand"] = np.array([r["n_cand"] for r in rows], np.int32)
    out["size"] = np.array([live, slots], np.int32)
    return out


def place_reference(c):
    ref, slot_of, slots, rows, reached = RP.PlaceRecognizerRef(c["n_words"]), {}, 0, [], set()
    for op in c["ops"]:
        if op[0] == "add":
            ref.add(op[1], op[2], op[3])
            slot_of[op[1]] = slots
            slots += 1
        elif op[0] == "erase":
            ref.erase(op[1])
        elif op[0] == "clear":
            ref.clear()
            slot_of, slots = {}, 0
        else:
            _, q, _, cap, _, tag = op
            keys, det = (ref.detect_reloc(q["query"][0], q["query"][1], c["neigh"]) if q["mode"] == "reloc" else
                         ref.detect_loop(q["query"][0], q["query"][1], q["connected"], q["min_score"], c["neigh"]))
            r = dict(n_cand=len(keys), cand=np.array([slot_of[k] for k in keys] if len(keys) <= cap else [], np.int32), words=np.full(slots, -1, np.int32),
                     score=np.zeros(slots, np.float32), acc=np.zeros(slots, np.float32), best=np.full(slots, -1, np.int32))
            for k in ref.bow:
                if k in det["words"]:
                    r["words"][slot_of[k]], r["score"][slot_of[k]] = det["words"][k], det["score"][k]
                if k in det["best"]:
                    r["acc"][slot_of[k]], r["best"][slot_of[k]] = det["acc"][k], slot_of[det["best"][k]]
            rows.append(r)
            reached |= {t for t in (tag, "cap below the candidates" if len(keys) > cap else None, None if keys else "no candidate") if t}
    return _place_pack(rows, len(ref.bow), slots), reached | {k for k, v in ref.trace.items() if v > 0}


def place_device(ctx, c):
    import ctypes as C
    import hyslam_amd as HS
    from devbuf import dev, out_buf, read
    from hyslam_amd import _native as N
    ex, s, lib = ctx.ex, ctx.stream(c["caller"]), ctx.ex._lib
    rec = HS.PlaceRecognizer(c["n_words"], ex)
    slot_all, rows, keep = {}, [], []                                 # key -> its latest slot, tombstones included: the library ignores those in a neighbour row
    pt = lambda a: a.ctypes.data_as(C.c_void_p)
    try:
        for op in c["ops"]:
            if op[0] == "add":
                _, key, w, v, on_device, slack, with_m = op
                if on_device:
                    m = len(w)
                    d_w, d_v = dev(np.concatenate([w, np.zeros(slack, np.int32)]).astype(np.int32)), dev(np.concatenate([v, np.zeros(slack)]).astype(np.float64))
                    d_m = dev(np.array([m], np.int32)) if with_m or slack else None
                    slot_all[key] = rec.add_device(key, d_w.ptr, d_v.ptr, d_m.ptr if d_m else None, m + slack, s.ptr or None)
                    s.synchronize()
                else:
                    slot_all[key] = rec.add(key, (w, v))
            elif op[0] == "erase":
                rec.erase(op[1])
            elif op[0] == "clear":
                rec.clear()
                slot_all = {}
            else:
                _, q, on_device, cap, with_m, _ = op
                slots = len(rec._keys)
                neigh = np.full((max(slots, 1), 10), -1, np.int32)
                for key, slot in rec._slot.items():
                    row = [slot_all[k] for k in list(c["neigh"].get(key, ()))[:10] if k in slot_all]
                    neigh[slot, :len(row)] = row
                excl = np.zeros(max(slots, 1), np.uint8)
                for k in q["connected"]:
                    if k in rec._slot:
                        excl[rec._slot[k]] = 1
                w, v = np.ascontiguousarray(q["query"][0], np.int32), np.ascontiguousarray(q["query"][1], np.float64)
                loop = q["mode"] == "loop"
                if on_device:
                    ins = [dev(w), dev(v), dev(np.array([len(w)], np.int32)) if with_m else None, dev(excl), dev(neigh)]
                    outs = [out_buf(4 * cap), out_buf(4)] + [out_buf(4 * slots) for _ in range(4)]
                    head = (rec._db, ins[0].ptr, ins[1].ptr, ins[2].ptr if ins[2] else None, len(w))
                    tail = (ins[4].ptr, outs[0].ptr, cap, outs[1].ptr, outs[2].ptr, outs[3].ptr, outs[4].ptr, outs[5].ptr, s.ptr or None)
                    st = lib.hs_place_query_loop_device(*head, ins[3].ptr, float(q["min_score"]), *tail) if loop else lib.hs_place_query_reloc_device(*head, *tail)
                    N.check(ex._h, st)
                    s.synchronize()
                    n = int(read(outs[1], np.int32, 1)[0])
                    cand = read(outs[0], np.int32, cap)
                    r = dict(n_cand=n, cand=cand[:n] if n <= cap else cand[cand != 0x55555555], words=read(outs[2], np.int32, slots), score=read(outs[3], np.float32, slots),
                             acc=read(outs[4], np.float32, slots), best=read(outs[5], np.int32, slots))
                else:
                    cand, n = np.full(max(cap, 1), 0x55555555, np.int32), C.c_int32()
                    o = dict(words=np.zeros(slots, np.int32), score=np.zeros(slots, np.float32), acc=np.zeros(slots, np.float32), best=np.zeros(slots, np.int32))
                    tail = (pt(neigh), pt(cand), cap, C.byref(n), pt(o["words"]), pt(o["score"]), pt(o["acc"]), pt(o["best"]))
                    st = (lib.hs_place_query_loop(rec._db, pt(w), pt(v), len(w), pt(excl), float(q["min_score"]), *tail) if loop else
                          lib.hs_place_query_reloc(rec._db, pt(w), pt(v), len(w), *tail))
                    assert st == (N.HS_OK if n.value <= cap else N.HS_ERR_CAPACITY), (st, n.value, cap)
                    r = dict(n_cand=n.value, cand=cand[:n.value] if n.value <= cap else cand[:cap][cand[:cap] != 0x55555555])
                    if st == N.HS_ERR_CAPACITY:                       # the host form stops there: the per-slot arrays come with the call a caller makes next
                        room, n2 = np.zeros(n.value, np.int32), C.c_int32()
                        tail = (pt(neigh), pt(room), n.value, C.byref(n2)) + tail[4:]
                        st = (lib.hs_place_query_loop(rec._db, pt(w), pt(v), len(w), pt(excl), float(q["min_score"]), *tail) if loop else
                              lib.hs_place_query_reloc(rec._db, pt(w), pt(v), len(w), *tail))
                        assert st == N.HS_OK and n2.value == n.value, (st, n2.value, n.value)
                    r.update(o)
                rows.append(r)
        live, slots = rec.size()
    finally:
        rec.close()
    return _place_pack(rows, live, slots)


# ================================================================ keyframe: the six hs_keyframe_*_device stages, each from what the previous one left
KEYFRAME_TAGS = ["insert", "no insert", "not ok", "depth walk cut", "n_new > new_cap", "held-but-unobserved view", "mono", "ref_slot outside"]
KF_RESULT_FIELDS = {1: ("ref_slot",), 2: ("ok",), 3: ("n_valid",), 4: ("n_ref_matches", "n_tracked_close", "n_nontracked_close", "insert"),
                    5: ("n_new", "n_candidates", "n_processed"), 6: ()}          # what each stage writes of hs_keyframe_result (chain_compare.compare_keyframe)
KF_RECORDS = ("new_view", "new_pos", "entries", "obs", "desc")


def keyframe_draw(rng, i):
    seed = int(rng.integers(0, 1 << 30))
    n, n_kf, sensor = max(1, draw_size(rng, 3000)), int(rng.integers(1, 7)), int(rng.random() < 0.8)
    L = int(rng.choice([3, max(3, n // 2), max(3, draw_size(rng, 20000))]))
    ref_kp = [None, 0, 1, 1025][int(rng.integers(0, 4))]
    prm = {}
    if rng.random() < 0.3:                                            # nothing asks for a key frame
        prm.update(frame_id=12, N_tracked_target=100, N_tracked_variance=10, min_N_tracked_close=0)
    if rng.random() < 0.15:
        prm.update(dict([[("ok_override", 0), ("force_loss", 1)][int(rng.integers(0, 2))]]))
    if rng.random() < 0.2:
        prm.update(force=1)
    c = KF.seeded(seed, n, L=L, n_kf=n_kf, ref_kp=ref_kp, sensor=sensor, **prm)
    if rng.random() < 0.2:
        c["ref_slot"] = int(rng.choice([-1, n_kf, n_kf + 3]))
    c["new_cap"] = draw_cap(rng, RKF.dense(c)["result"]["n_new"])
    c["what"] = params(seed=seed, n=n, L=L, n_kf=n_kf, ref_kp=ref_kp, sensor=sensor, ref_slot=c["ref_slot"], new_cap=c["new_cap"], **prm)
    return c


def _keyframe_outputs(got, stage, new_cap, n_new=None):
    """one stage's outputs under the names the comparison reports; got: Dev.results() or the reference's dict"""
    r = got["result"][0] if isinstance(got["result"], np.ndarray) else got["result"]
    out = {"s%d.result.%s" % (stage, k): int(r[k]) for k in KF_RESULT_FIELDS[stage]}
    out["s%d.ref_slot" % stage] = got["ref_slot_mem"] if "ref_slot_mem" in got else r["ref_slot"]
    for k in ("kp_lm", "kp_outl", "n_matches", "kp_lm_obs"):
        out["s%d.%s" % (stage, k)] = got[k]
    if stage == 5:
        device = n_new is not None
        m = min(n_new if device else r["n_new"], new_cap)
        out["s5.pose_view"] = np.frombuffer(np.asarray(got["pose_view"]).tobytes(), np.uint8)
        for k in KF_RECORDS:
            a = np.ascontiguousarray(got[k])
            rows = a.view(np.uint8).reshape(new_cap, -1) if device and new_cap else a[:m].view(np.uint8).reshape(m, -1) if m else np.zeros((0, 1), np.uint8)
            out["s5." + k] = rows[:m].reshape(-1)
            out["s5.%s.behind" % k] = int(device and bool((rows[m:] != 0x55).any()))      # nothing behind the last record: the fill pattern is still there
        out["s5.lm_index"] = got["lm_index"]
        out["s5.obs_offsets"], out["s5.desc_offsets"] = (got["obs_offsets"], got["desc_offsets"]) if device else (got["offsets"], got["offsets"])
    return out


def keyframe_reference(c):
    want, cur, res, nm = {}, dict(c), {k: 0 for k in RKF.RESULT_KEYS}, {}
    for s in range(1, 7):
        w = RKF.dense(cur, stages=(s,), res=res)
        want.update(_keyframe_outputs(w, s, c["new_cap"]))
        cur = dict(cur, state=(w["kp_lm"], w["kp_outl"], w["n_matches"]), ref_slot=w["result"]["ref_slot"], kp_lm_obs=w["kp_lm_obs"])
        res, nm[s] = w["result"], w["n_matches"]
    reached = {"insert" if res["insert"] else "no insert"} | {t for t, hit in (
        ("not ok", not res["ok"]), ("depth walk cut", res["n_processed"] < res["n_candidates"]), ("n_new > new_cap", res["n_new"] > c["new_cap"]),
        ("held-but-unobserved view", nm[3] < nm[2]), ("mono", c["frame"]["sensor"] == 0), ("ref_slot outside", not 0 <= res["ref_slot"] < c["K"]["n_kf"])) if hit}
    return want, reached


def keyframe_device(ctx, c):
    from test_gpu_keyframe import Dev, put
    d, got = Dev(ctx.tracker, c), {}
    put(d.obufs["result"][0], np.zeros(1, d.N.KEYFRAME_RESULT_DTYPE))
    n_new = 0
    for s in range(1, 7):
        d.stage(s)
        g = d.results()
        n_new = int(g["result"][0]["n_new"]) if s >= 5 else n_new
        got.update(_keyframe_outputs(g, s, c["new_cap"], n_new=max(n_new, 0)))
    return got


def keyframe_exhaustive(ctx, stride=1, report=None):
    """the three exhaustive spaces of tests/test_keyframe_ref.py (~22 500 cases), every stride-th, stage by stage -> (cases, first mismatch or None)"""
    import test_keyframe_ref as TK
    count = 0
    for j, (tag, c) in enumerate(TK.exhaustive_cases()):
        if j % stride:
            continue
        want, _ = keyframe_reference(c)
        good, bad = compare(want, keyframe_device(ctx, c))
        count += 1
        if not good:
            return count, "keyframe exhaustive case %d %s: MISMATCH in %s" % (j, tag, ", ".join(bad))
    return count, None


# ================================================================ bow_kf: hs_search_by_bow_kf_device
BOW_KF_TAGS = ["match", "two key-frame keypoints take one view", "kf_cap truncates", "slot outside", "empty key frame", "weights on the device", "nodes masked"]
BOW_KF_OUT = ("match_kf", "op_view", "op_lm", "n_matches")


def bow_kf_draw(rng, i):
    seed = int(rng.integers(0, 1 << 30))
    n, L, n_nodes = max(1, draw_size(rng, 3000)), max(1, draw_size(rng, 20000)), int(rng.choice([1, 3, 40, 500]))
    kf_sizes = [draw_size(rng, 2200) for _ in range(int(rng.integers(1, 4)))]
    dens = dict(p_lm=float(rng.choice([0.0, 0.5, 0.9, 1.0])), p_bad=float(rng.choice([0.0, 0.05, 0.5])), p_twin=float(rng.choice([0.0, 0.3, 0.9])),
                p_turned=float(rng.choice([0.0, 0.15, 0.6])), max_flip=int(rng.choice([0, 14, 40])))
    K, lm_bad, fkps, fdesc, fnode, fweight = RC.random_search(seed, n, kf_sizes, L, n_nodes, **dens)
    slot = int(rng.integers(0, len(kf_sizes))) if rng.random() < 0.85 else int(rng.choice([-1, len(kf_sizes), len(kf_sizes) + 7]))
    size = kf_sizes[slot] if 0 <= slot < len(kf_sizes) else 0
    kf_cap = max(1, draw_cap(rng, size))
    th_low, nnratio = float(rng.choice([50.0, 30.0, 100.0])), float(np.float32(rng.choice([0.6, 0.7, 0.9, 1.0])))
    return dict(K=K, lm_bad=lm_bad, L=L, fkps=fkps, fdesc=fdesc, fnode=fnode, fweight=fweight, slot=slot, size=size, kf_cap=kf_cap, th_low=th_low, nnratio=nnratio,
                with_weight=bool(rng.integers(0, 2)),
                what=params(seed=seed, n=n, L=L, n_nodes=n_nodes, kf_sizes=kf_sizes, **dens, slot=slot, kf_cap=kf_cap, th_low=th_low, nnratio=nnratio))


def bow_kf_reference(c):
    masked = np.where(c["fweight"] > 0, c["fnode"], -1).astype(np.int32)
    w = RR.search_by_bow_kf_dense(c["K"], c["slot"], c["kf_cap"], c["L"], c["lm_bad"], c["fkps"], c["fdesc"], c["fnode"] if c["with_weight"] else masked,
                                  c["fweight"] if c["with_weight"] else None, c["th_low"], c["nnratio"])
    live = w[0][w[0] >= 0]
    reached = {"weights on the device" if c["with_weight"] else "nodes masked"} | {t for t, hit in (
        ("match", w[3] > 0), ("two key-frame keypoints take one view", len(np.unique(live)) < len(live)), ("kf_cap truncates", c["size"] > c["kf_cap"]),
        ("slot outside", not 0 <= c["slot"] < c["K"]["n_kf"]), ("empty key frame", 0 <= c["slot"] < c["K"]["n_kf"] and c["size"] == 0)) if hit}
    return dict(zip(BOW_KF_OUT, w)), reached


def bow_kf_device(ctx, c):
    from test_gpu_refkf import search_device
    masked = np.where(c["fweight"] > 0, c["fnode"], -1).astype(np.int32)
    got = search_device(ctx.tracker, c["K"], c["slot"], c["kf_cap"], c["lm_bad"], c["L"], c["fkps"], c["fdesc"], c["fnode"] if c["with_weight"] else masked,
                        c["th_low"], c["nnratio"], c["fweight"] if c["with_weight"] else None)
    return dict(zip(BOW_KF_OUT, got))


# ================================================================ the families
class Family:
    def __init__(self, name, tags, draw, reference, device, seed, cases):
        self.name, self.tags, self.draw, self.reference, self.device = name, tags, draw, reference, device
        self.seed, self.cases = seed, cases                          # the committed slice of tests/test_gpu_fuzz_map.py: every tag reached (test_fuzz_map_cases.py)

    def describe(self, c, i, seed):
        return "%s --seed %s case %d: %s" % (self.name, seed, i, c["what"])

    def one_case(self, rng, i, ctx):
        """-> (message, good, reached).  The message of a mismatch replays the case: family, seed, case index, drawn parameters"""
        c = self.draw(rng, i)
        want, reached = self.reference(c)
        good, bad = compare(want, self.device(ctx, c))
        return self.describe(c, i, getattr(ctx, "seed", "?")) + (" -> ok" if good else " -> MISMATCH in %s" % ", ".join(bad)), good, reached

    def reach(self, seed=None, cases=None):
        """generator + reference only: the tags `cases` cases of `seed` reach, as a counter"""
        rng, seen = np.random.default_rng(self.seed if seed is None else seed), {}
        for i in range(self.cases if cases is None else cases):
            for t in self.reference(self.draw(rng, i))[1]:
                seen[t] = seen.get(t, 0) + 1
        return seen


def both(tags):
    return ["%s: %s" % (w, t) for w in ("lm", "vw") for t in tags]


FAMILIES = {f.name: f for f in (
    Family("landmark_descriptors", DESC_TAGS, desc_draw, desc_reference, desc_device, seed=1, cases=24),
    Family("landmark_entries", ENTRY_TAGS, entries_draw, entries_reference, entries_device, seed=1, cases=24),
    Family("place", PLACE_TAGS, place_draw, place_reference, place_device, seed=1, cases=12),
    Family("local_map", LOCAL_TAGS, local_draw, local_reference, local_device, seed=2, cases=24),
    Family("kf_votes", VOTES_TAGS, votes_draw, votes_reference, votes_device, seed=1, cases=24),
    Family("kf_redundancy", RED_TAGS, red_draw, red_reference, red_device, seed=1, cases=24),
    Family("keyframe", KEYFRAME_TAGS, keyframe_draw, keyframe_reference, keyframe_device, seed=1, cases=16),
    Family("bow_kf", BOW_KF_TAGS, bow_kf_draw, bow_kf_reference, bow_kf_device, seed=1, cases=16),
    Family("replay", both(REPLAY_TAGS), replay_draw, replay_reference, replay_device, seed=1, cases=24),
    Family("frame_state", FRAME_STATE_TAGS, frame_state_draw, frame_state_reference, frame_state_device, seed=2, cases=24),
)}


def summary(paths):
    """the campaign's logs -> the text of profiles/fuzz_map_campaign.txt: cases per family, how often each tag was reached, every mismatch line"""
    import re
    cases, tags, bad, runs, extra, seeds = {}, {}, [], 0, [], []
    for path in paths:
        for line in open(path):
            line = line.rstrip("\n")
            m = re.match(r"tags (\w+) \((\d+) cases\): (.*)", line)
            if m:
                cases[m.group(1)] = cases.get(m.group(1), 0) + int(m.group(2))
                for item in m.group(3).split("; "):
                    t, k = item.rsplit(" ", 1)
                    tags[(m.group(1), t)] = tags.get((m.group(1), t), 0) + int(k)
            elif "MISMATCH" in line or "differs" in line:
                bad.append(line)
            elif line.startswith("fuzz map: seed"):
                runs += 1
                seeds.append(int(line.split()[3].rstrip(",")))
            elif "exhaustive" in line and not line.startswith("fuzz map"):
                extra.append(line)
    out = ["map-side fuzz campaign (tools/fuzz_map.py --family all --seed S; seeds %s): %d runs, %d cases, %d mismatches" % (
        ", ".join(map(str, sorted(seeds))), runs, sum(cases.values()), len(bad)), "per family: cases, then in how many of them the reference's result reached each tag", ""]
    for name, fam in FAMILIES.items():
        out.append("%s: %d cases" % (name, cases.get(name, 0)))
        out += ["    %-45s %d%s" % (t, tags.get((name, t), 0), "" if tags.get((name, t), 0) else "   NEVER REACHED") for t in fam.tags]
    out += ["", "exhaustive spaces:"] + ["    " + e for e in extra] + ["", "mismatches:"] + (["    " + b for b in bad] or ["    none"])
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", default="all", help="|".join(FAMILIES) + "|all")
    ap.add_argument("--cases", type=int, default=40)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--exhaustive", type=int, nargs="*", metavar="N L", help="--family replay --exhaustive N L: both replays over the whole N x L space; "
                    "--family keyframe --exhaustive: the three exhaustive spaces of tests/test_keyframe_ref.py, stage by stage")
    ap.add_argument("--stride", type=int, default=1, help="with --exhaustive: every stride-th case")
    ap.add_argument("--tags", action="store_true", help="generator and reference only: count the tags, touch no device")
    ap.add_argument("--summary", nargs="+", metavar="LOG", help="summarise logs of this tool (profiles/fuzz_map_campaign.txt) and exit")
    a = ap.parse_args()
    if a.summary:
        sys.stdout.write(summary(a.summary))
        return
    names = list(FAMILIES) if a.family == "all" else [a.family]
    t0, bad, seen, ran = time.time(), 0, {}, {}
    ctx = Context(a.seed)
    if a.exhaustive is not None:
        if a.family == "keyframe":
            count, msg = keyframe_exhaustive(ctx, a.stride)
            print(msg or "keyframe exhaustive spaces, stride %d: %d cases ok, %.1f s" % (a.stride, count, time.time() - t0), flush=True)
            bad += msg is not None
        else:
            n, L = a.exhaustive
            for which in ("lm", "vw"):
                t1 = time.time()
                count, msg = exhaustive_check(which, n, L, device_runner(ctx, which), a.seed, stride=a.stride)
                print(msg or "replay %s exhaustive %d x %d, stride %d: %d cases ok, %.1f s" % (which, n, L, a.stride, count, time.time() - t1), flush=True)
                bad += msg is not None
        print("fuzz map: exhaustive spaces, %d mismatches, %.0f s" % (bad, time.time() - t0))
        sys.exit(1 if bad else 0)
    for name in names:
        fam, rng = FAMILIES[name], np.random.default_rng(a.seed)
        for i in range(a.cases):
            if a.tags:
                c = fam.draw(rng, i)
                msg, good, reached = fam.describe(c, i, a.seed), True, fam.reference(c)[1]
            else:
                msg, good, reached = fam.one_case(rng, i, ctx)
            print(msg, flush=True)
            ran[name] = ran.get(name, 0) + 1
            for t in reached:
                seen[(name, t)] = seen.get((name, t), 0) + 1
            bad += not good
            if not good:
                break
        if bad:
            break
    for name in names:
        print("tags %s (%d cases): %s" % (name, ran.get(name, 0), "; ".join("%s %d" % (t, seen.get((name, t), 0)) for t in FAMILIES[name].tags)))
    print("fuzz map: seed %d, %d cases, %d mismatches, %.0f s" % (a.seed, sum(ran.values()), bad, time.time() - t0))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
