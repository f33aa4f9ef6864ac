"""CPU: what the resident tracking chain rests on (tests/ref_track.py, tests/track_cases.py).

  * the replay's closed form (the numpy twin of kernels_track.hip's k_assoc_* phases) against the sequential LandMarkMatches restatement —
    EXHAUSTIVELY over every initial state and every op set with up to 4 views and up to 4 landmarks (duplicated landmarks, all three flag values
    on every view, ops onto their own view), then on randomised states of up to 130 views: the proof the kernel's algorithm rests on
  * the dense model against the map-based LandMarkMatches, op by op and over the whole chain on the directed cases
  * the pose view against pyref's gemm and the float product of oracle.make_frame_view
  * the directed cases hold by construction, and the random cases qualify within the rejection cap
"""
import itertools

import numpy as np
import pytest

import pyref
import ref_track as R
import track_cases as TC

NONE = R.NONE


# ---- batched restatements for the exhaustive enumeration: state [B, n], opv [B, L] = the view op k targets, -1 = landmark k has no op
def seq_batch(kp, outl, nm, opv):
    """LandMarkMatches::associateLandMark(opv[k], k, true) for k ascending, literally, on B states at once"""
    kp, outl, nm = kp.copy(), outl.copy(), nm.copy()
    ar = np.arange(len(kp))
    for k in range(opv.shape[1]):
        v = opv[:, k]
        act = v >= 0
        vi = np.where(act, v, 0)
        holds = kp == k
        j = np.where(holds.any(1), holds.argmax(1), -1)            # hasAssociation(pMP): the first view in map order
        old = kp[ar, vi] >= 0                                       # hasAssociation(i)
        fresh = act & ~old & (j < 0)
        repl = act & ~fresh
        o = outl[fresh, vi[fresh]]
        kp[fresh, vi[fresh]] = k
        outl[fresh, vi[fresh]] = np.where(o == 0, 1, o)             # insert: no overwrite
        nm[fresh] += 1
        kp[repl, vi[repl]] = k
        outl[repl, vi[repl]] = 1
        er = repl & (j >= 0) & (j != vi)
        kp[er, j[er]] = -1
    return kp, outl, nm


def closed_batch(kp0, outl, nm, opv, strict=False):
    """ref_track.replay_closed_form's phases on B states at once"""
    B, n = kp0.shape
    L = opv.shape[1]
    ar = np.arange(B)
    minw, maxw = np.full((B, n), NONE, np.int64), np.full((B, n), -1, np.int64)
    for k in range(L):
        a = opv[:, k] >= 0
        maxw[a, opv[a, k]] = k
    for k in reversed(range(L)):
        a = opv[:, k] >= 0
        minw[a, opv[a, k]] = k
    holds = (kp0 >= 0) & ((minw > kp0) if strict else (minw >= kp0))
    jk = np.full((B, L), NONE, np.int64)
    for k in range(L):
        m = holds & (kp0 == k)
        jk[:, k] = np.where(m.any(1), m.argmax(1), NONE)
    erased = np.zeros((B, n), bool)
    for k in range(L):
        v = opv[:, k]
        hit = (v >= 0) & (jk[:, k] != NONE) & (jk[:, k] != v)
        erased[hit, jk[hit, k]] = True
    written = maxw >= 0
    first = np.where(written, minw, 0)
    fresh = written & ((kp0 < 0) | erased) & (np.take_along_axis(jk, first, 1) == NONE)
    out = np.where(written, maxw, np.where(erased, -1, kp0))
    keep = fresh & (minw == maxw) & (outl != 0)
    outl2 = np.where(written & ~keep, 1, outl)
    return out, outl2, nm + fresh.sum(1)


def state_tables(n, L):
    """the factors of the enumeration: kp_lm in {-1 .. L-1}^n, kp_outl in {0, 1, 2}^n (every flag on every view: a stale `false` entry on an empty view
    is what a moved landmark leaves, a held view without an entry cannot arise but costs nothing), ops in {-1 .. n-1}^L"""
    kp = np.array(list(itertools.product(range(-1, L), repeat=n)), np.int64).reshape(-1, n)
    fl = np.array(list(itertools.product(range(3), repeat=n)), np.uint8).reshape(-1, n)
    op = np.array(list(itertools.product(range(-1, n), repeat=L)), np.int64).reshape(-1, L)
    return kp, fl, op


def enumerate_states(n, L, chunk=1 << 20):
    """yields (first index, kp_lm, kp_outl, ops) over the full product of state_tables, `chunk` states at a time"""
    kp, fl, op = state_tables(n, L)
    total = len(kp) * len(fl) * len(op)
    for s in range(0, total, chunk):
        idx = np.arange(s, min(s + chunk, total))
        yield s, kp[idx // (len(fl) * len(op))], fl[(idx // len(op)) % len(fl)], op[idx % len(op)]


@pytest.mark.parametrize("n,L", [(1, 1), (1, 4), (2, 2), (2, 4), (3, 3), (4, 2), (3, 4), (4, 3), (4, 4)])
def test_replay_closed_form_exhaustive(n, L):
    """EVERY initial state and op set: (L + 1)^n landmarks x 3^n flags x (n + 1)^L ops — 31.6 million at 4 x 4"""
    count = 0
    for s, k0, f0, o0 in enumerate_states(n, L):
        nm = (np.arange(s, s + len(k0)) % 5).astype(np.int64)
        want, got = seq_batch(k0, f0, nm, o0), closed_batch(k0, f0, nm, o0)
        for w, g, what in zip(want, got, ("kp_lm", "kp_outl", "n_matches")):
            bad = np.nonzero((w != g).reshape(len(k0), -1).any(1))[0]
            assert len(bad) == 0, (what, k0[bad[0]], f0[bad[0]], o0[bad[0]], w[bad[0]], g[bad[0]])
        count += len(k0)
    assert count == (L + 1) ** n * 3 ** n * (n + 1) ** L


def test_batched_restatements_are_the_module_functions():
    """the exhaustive test runs batched twins: on a sample of its states they equal ref_track's MapMatches loop and replay_closed_form"""
    _, kp, fl, op = next(enumerate_states(3, 3, chunk=1 << 30))
    pick = np.arange(7, len(kp), 997)
    nm = np.arange(len(pick))
    ws, wc = seq_batch(kp[pick], fl[pick], nm, op[pick]), closed_batch(kp[pick], fl[pick], nm, op[pick])
    for r, i in enumerate(pick):
        ops_lm = np.nonzero(op[i] >= 0)[0]
        ops_v = op[i][ops_lm]
        m = R.replay_sequential(R.MapMatches.from_dense(kp[i], fl[i], nm[r]), ops_v, ops_lm, 3, 3).dense(3)
        c = R.replay_closed_form(kp[i], fl[i], nm[r], ops_v, ops_lm, 3)
        for a, b, x, y in zip(m, c, (ws[0][r], ws[1][r], ws[2][r]), (wc[0][r], wc[1][r], wc[2][r])):
            assert np.array_equal(a, x) and np.array_equal(b, y) and np.array_equal(a, b)


REPLAY_SIZES = [(1, 1), (5, 9), (63, 64), (64, 63), (65, 130), (130, 65), (130, 130), (100, 300)]


@pytest.mark.parametrize("n,n_ops", REPLAY_SIZES)
def test_replay_randomised(n, n_ops):
    """closed form == dense model == the maps, on states with duplicates, stale entries, ops onto the landmark's own view and moving landmarks"""
    seen = dict(fresh=0, moves=0, stale=0, own=0)
    for seed in range(40):
        s = TC.replay_state(1000 * n + seed, n, n_ops)
        maps = R.replay_sequential(R.MapMatches.from_dense(s["kp_lm"], s["kp_outl"], s["n_matches"]), s["op_view"], s["op_lm"], n, s["L"]).dense(n)
        dense = R.replay_sequential(R.DenseMatches.from_dense(s["kp_lm"], s["kp_outl"], s["n_matches"]), s["op_view"], s["op_lm"], n, s["L"]).dense(n)
        closed = R.replay_closed_form(s["kp_lm"], s["kp_outl"], s["n_matches"], s["op_view"], s["op_lm"], s["L"])
        for a, b, c in zip(maps, dense, closed):
            assert np.array_equal(a, b) and np.array_equal(a, c), (n, n_ops, seed)
        ok = R.valid_ops(s["op_view"], s["op_lm"], n, s["L"])
        seen["fresh"] += maps[2] - s["n_matches"]
        seen["moves"] += int(((s["kp_lm"] >= 0) & (maps[0] == -1)).sum())
        seen["stale"] += int(((s["kp_lm"] < 0) & (s["kp_outl"] == 2) & (maps[1] == 2) & (maps[0] >= 0)).sum())
        seen["own"] += int((s["kp_lm"][s["op_view"][ok]] == s["op_lm"][ok]).sum())
    if n >= 63:
        assert all(v > 0 for v in seen.values()), seen


def test_replay_mutations_are_visible():
    """the two mutations of the algorithm that the issue names change the result on these states: ops in array order; minw[u] > k for >="""
    order = strict = 0
    for seed in range(60):
        s = TC.replay_state(555000 + seed, 40, 60)
        want = R.replay_closed_form(s["kp_lm"], s["kp_outl"], s["n_matches"], s["op_view"], s["op_lm"], s["L"])
        m = R.DenseMatches.from_dense(s["kp_lm"], s["kp_outl"], s["n_matches"])
        for j in np.nonzero(R.valid_ops(s["op_view"], s["op_lm"], 40, s["L"]))[0]:             # array order
            m.associate(int(s["op_view"][j]), int(s["op_lm"][j]))
        order += any(not np.array_equal(a, b) for a, b in zip(want, m.dense()))
        got = R.replay_closed_form(s["kp_lm"], s["kp_outl"], s["n_matches"], s["op_view"], s["op_lm"], s["L"], minw_strict=True)
        strict += any(not np.array_equal(a, b) for a, b in zip(want, got))
    assert order > 10 and strict > 5, (order, strict)


def test_pose_view():
    import oracle
    from hyslam_amd import _native as N
    differs = 0
    for seed in range(50):
        rng = np.random.default_rng(seed)
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        T[:3, 3] = rng.normal(0, 3, 3)
        pv = R.pose_view(T)
        assert pv["Rcw"].tobytes() == T[:3, :3].tobytes() and pv["tcw"].tobytes() == T[:3, 3].tobytes() and pv.nbytes == 64
        for i in range(3):
            exact = -(float(T[0, i]) * float(T[0, 3]) + float(T[1, i]) * float(T[1, 3]) + float(T[2, i]) * float(T[2, 3]))
            assert pv["Ow"][i] == np.float32(exact)                  # one rounding of the double sum
        F, keep = oracle.make_frame_view(N.FrameView, T[:3, :3], T[:3, 3], 500, 500, 320, 240, 60, 1, (0, 640, 0, 480), np.zeros(1, N.KP_DTYPE), np.zeros((1, 32), np.uint8))
        assert np.allclose(np.array(F.Ow[:]), pv["Ow"], rtol=0, atol=4e-6 * float(np.abs(T[:3, 3]).sum()))
        differs += R.pose_view_float(T)["Ow"].tobytes() != pv["Ow"].tobytes()
    assert differs > 5                                               # a float accumulation is a different function: the GPU test's poses include such


def test_directed_cases_hold_and_chain_dense_equals_maps():
    for name in TC.DIRECTED:
        if name == "chunk_1025":
            continue                                                 # the same code on a larger frame: the GPU test builds it
        c, (m, l) = TC.directed(name)                                # asserts the directed property and the qualification
        n = len(c["frame"]["kps"])
        m2, l2 = R.track_frame(c, R.MapMatches())
        for a, b in ((m, m2), (l, l2)):
            for k in ("after_associate", "state"):
                for x, y in zip(a[k], b[k]):
                    assert np.array_equal(x, y), (name, k)
            assert a["pose"]["Tcw_d"].tobytes() == b["pose"]["Tcw_d"].tobytes() and a["n_edges"] == b["n_edges"], name
        assert (m["n_matches_map"], l["n_inliers"]) == (m2["n_matches_map"], l2["n_inliers"]), name
        assert l["state"][2] == int((l["state"][0] >= 0).sum()) or name                       # n_matches is path dependent; equal here: nothing moves


def test_sensor_decides_what_the_local_stage_removes():
    (c0, (_, l0)), (c1, (_, l1)) = TC.directed("mono_keeps_outliers"), TC.directed("stereo_removes_outliers")
    out0 = l0["pose"]["outlier"].astype(bool)
    assert (l0["state"][0][l0["edges"]["kp"][out0]] >= 0).all() and (l0["state"][1][l0["edges"]["kp"][out0]] == 2).all()
    out1 = l1["pose"]["outlier"].astype(bool)
    assert (l1["state"][0][l1["edges"]["kp"][out1]] == -1).all() and (l1["state"][1][l1["edges"]["kp"][out1]] == 0).all()


def test_random_cases_qualify_within_the_cap():
    cases, drawn = TC.random_cases()
    assert len(cases) == TC.N_RANDOM and drawn <= 2 * TC.N_RANDOM
    assert any(c["frame"]["sensor"] == 0 for c, _ in cases) and any(c["frame"]["sensor"] == 1 for c, _ in cases)
