"""CPU: what the resident first stage of the tracker rests on (tests/ref_refkf.py, tests/refkf_cases.py).

  * the closed form of the replay in VIEW order (the numpy twin of kernels_track_refkf.hip's k_vassoc_* phases) against the sequential
    LandMarkMatches restatement — EXHAUSTIVELY over every initial state and every valid op set (a view in at most one op, a landmark in at most one)
    with up to 4 views and up to 4 landmarks, landmarks duplicated in the initial state and all three flag values on every view included; then on
    randomised states of up to 300 views
  * the literal restatement (dicts walked as the std::maps) against the dense one (the device layout) on every directed and random case: the
    search, the associations, the optimiser's input and result, the gates, the counts
  * the directed cases hold by construction, and at least three quarters of the seeded cases qualify"""
import itertools

import numpy as np
import pytest

import ref_refkf as RR
import ref_track as R
import refkf_cases as RC

NONE = RR.NONE


# ---- batched restatements for the exhaustive enumeration: state [B, n], opl [B, n] = the landmark of the view's op, -1 = none
def seq_batch(kp, outl, nm, opl):
    """LandMarkMatches::associateLandMark(v, opl[v], true) for v ascending, literally, on B states at once"""
    kp, outl, nm = kp.copy(), outl.copy(), nm.copy()
    for v in range(opl.shape[1]):
        m = opl[:, v]
        act = m >= 0
        holds = kp == m[:, None]
        j = np.where(act & holds.any(1), holds.argmax(1), -1)         # hasAssociation(pMP): the first view in map order
        old = kp[:, v] >= 0                                            # hasAssociation(i)
        fresh = act & ~old & (j < 0)
        repl = act & ~fresh
        o = outl[fresh, v]
        kp[fresh, v] = m[fresh]
        outl[fresh, v] = np.where(o == 0, 1, o)                        # insert: no overwrite
        nm[fresh] += 1
        kp[repl, v] = m[repl]
        outl[repl, v] = 1
        er = repl & (j >= 0) & (j != v)
        kp[er, j[er]] = -1
    return kp, outl, nm


def closed_batch(kp0, outl, nm, opl, L):
    """ref_refkf.replay_views_closed_form's phases on B states at once"""
    B, n = kp0.shape
    ar, views = np.arange(B), np.arange(n)[None, :]
    lm_view = np.full((B, L), NONE, np.int64)
    for v in range(n):
        a = opl[:, v] >= 0
        lm_view[a, opl[a, v]] = v
    held = kp0 >= 0
    k = np.where(held, kp0, 0)
    lv = np.take_along_axis(lm_view, k, 1)                              # the view of the op of the landmark each view holds
    holder = held & (lv != NONE) & ((opl < 0) | (views >= lv))
    idx_old = np.full((B, L), NONE, np.int64)
    for m in range(L):
        h = holder & (kp0 == m)
        idx_old[:, m] = np.where(h.any(1), h.argmax(1), NONE)
    erased = held & (lv != NONE) & (np.take_along_axis(idx_old, k, 1) == views)
    has_op = opl >= 0
    fresh = has_op & (~held | (erased & (lv < views))) & (np.take_along_axis(idx_old, np.where(has_op, opl, 0), 1) == NONE)
    out = np.where(has_op, opl, np.where(erased, -1, kp0))
    outl2 = np.where(has_op & ~(fresh & (outl != 0)), 1, outl)
    return out, outl2, nm + fresh.sum(1)


def state_tables(n, L):
    """the factors of the enumeration: kp_lm in {-1 .. L-1}^n, kp_outl in {0, 1, 2}^n, and the op sets: a landmark or none per view, no landmark twice"""
    kp = np.array(list(itertools.product(range(-1, L), repeat=n)), np.int64).reshape(-1, n)
    fl = np.array(list(itertools.product(range(3), repeat=n)), np.uint8).reshape(-1, n)
    op = np.array([o for o in itertools.product(range(-1, L), repeat=n) if len({x for x in o if x >= 0}) == sum(x >= 0 for x in o)], np.int64).reshape(-1, n)
    return kp, fl, op


def enumerate_states(n, L, chunk=1 << 20):
    kp, fl, op = state_tables(n, L)
    total = len(kp) * len(fl) * len(op)
    for s in range(0, total, chunk):
        idx = np.arange(s, min(s + chunk, total))
        yield s, kp[idx // (len(fl) * len(op))], fl[(idx // len(op)) % len(fl)], op[idx % len(op)]


def n_op_sets(n, L):
    from math import comb, perm
    return sum(comb(n, k) * perm(L, k) for k in range(min(n, L) + 1))


@pytest.mark.parametrize("n,L", [(1, 1), (1, 4), (2, 2), (2, 4), (3, 3), (4, 2), (3, 4), (4, 3), (4, 4)])
def test_view_order_closed_form_exhaustive(n, L):
    """EVERY initial state and valid op set: (L + 1)^n landmarks x 3^n flags x (partial injections of views into landmarks) — 10.6 million at 4 x 4"""
    count = 0
    for s, k0, f0, o0 in enumerate_states(n, L):
        nm = (np.arange(s, s + len(k0)) % 5).astype(np.int64)
        want, got = seq_batch(k0, f0, nm, o0), closed_batch(k0, f0, nm, o0, L)
        for w, g, what in zip(want, got, ("kp_lm", "kp_outl", "n_matches")):
            bad = np.nonzero((w != g).reshape(len(k0), -1).any(1))[0]
            assert len(bad) == 0, (what, k0[bad[0]], f0[bad[0]], o0[bad[0]], w[bad[0]], g[bad[0]])
        count += len(k0)
    assert count == (L + 1) ** n * 3 ** n * n_op_sets(n, L)


def test_batched_restatements_are_the_module_functions():
    """the exhaustive test runs batched twins: on a sample of its states they equal the MapMatches loop and ref_refkf.replay_views_closed_form"""
    _, kp, fl, op = next(enumerate_states(3, 3, chunk=1 << 30))
    pick = np.arange(7, len(kp), 499)
    nm = np.arange(len(pick))
    ws, wc = seq_batch(kp[pick], fl[pick], nm, op[pick]), closed_batch(kp[pick], fl[pick], nm, op[pick], 3)
    for r, i in enumerate(pick):
        ov = np.arange(3)[::-1]                                         # array order is not view order
        m = RR.replay_views_sequential(R.MapMatches.from_dense(kp[i], fl[i], nm[r]), ov, op[i][ov], 3, 3).dense(3)
        c = RR.replay_views_closed_form(kp[i], fl[i], nm[r], ov, op[i][ov], 3)
        for a, b, x, y in zip(m, c, (ws[0][r], ws[1][r], ws[2][r]), (wc[0][r], wc[1][r], wc[2][r])):
            assert np.array_equal(a, x) and np.array_equal(b, y) and np.array_equal(a, b)


@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 130, 300])
def test_view_order_replay_randomised(n):
    """closed form == dense model == the maps, on states with duplicates, stale entries, ops onto the landmark's own view and moving landmarks; and
    the landmark-order replay of the motion stage is a different function on the same ops"""
    seen = dict(fresh=0, moves=0, stale=0, own=0, differs=0)
    for seed in range(40):
        s = RC.replay_state(2000 * n + seed, n)
        args = (s["op_view"], s["op_lm"], n, s["L"])
        maps = RR.replay_views_sequential(R.MapMatches.from_dense(s["kp_lm"], s["kp_outl"], s["n_matches"]), *args).dense(n)
        dense = RR.replay_views_sequential(R.DenseMatches.from_dense(s["kp_lm"], s["kp_outl"], s["n_matches"]), *args).dense(n)
        closed = RR.replay_views_closed_form(s["kp_lm"], s["kp_outl"], s["n_matches"], s["op_view"], s["op_lm"], s["L"])
        for a, b, c in zip(maps, dense, closed):
            assert np.array_equal(a, b) and np.array_equal(a, c), (n, seed)
        ok = R.valid_ops(*args)
        assert len(np.unique(s["op_view"][ok])) == ok.sum() == len(np.unique(s["op_lm"][ok]))          # the preconditions
        other = R.replay_sequential(R.MapMatches.from_dense(s["kp_lm"], s["kp_outl"], s["n_matches"]), *args).dense(n)
        seen["differs"] += any(not np.array_equal(a, b) for a, b in zip(maps, other))
        seen["fresh"] += maps[2] - s["n_matches"]
        seen["moves"] += int(((s["kp_lm"] >= 0) & (maps[0] == -1)).sum())
        seen["stale"] += int(((s["kp_lm"] < 0) & (s["kp_outl"] == 2) & (maps[1] == 2) & (maps[0] >= 0)).sum())
        seen["own"] += int((s["kp_lm"][s["op_view"][ok]] == s["op_lm"][ok]).sum())
    if n >= 63:
        assert all(v > 0 for v in seen.values()), seen


def _literal(c, vv):
    return RR.track_normal(c, vv, R.MapMatches.from_dense(*c["state0"]))


def check_literal_equals_dense(c, vv, ref, tag):
    motion, rk, local = ref
    init, llocal = _literal(c, vv)
    n = len(c["frame"]["kps"])
    lit = init["refkf"]
    status = int(rk["result"]["refkf_status"][0])
    assert (lit is None) == (status == RR.REFKF_SKIPPED), tag
    if lit is not None:
        assert lit["n_bow"] == rk["result"]["n_bow"][0], tag
        assert lit["internal"] == {int(j): int(f) for j, f in enumerate(rk["match_kf"]) if f >= 0}, tag
        assert lit["matches_bow"] == {int(f): int(rk["op_lm"][f]) for f in np.nonzero(rk["op_view"] >= 0)[0]}, tag
        assert (rk["op_view"][rk["op_view"] >= 0] == np.nonzero(rk["op_view"] >= 0)[0]).all() and ((rk["op_view"] < 0) == (rk["op_lm"] < 0)).all(), tag
        assert (lit["ret"] == -1) == (status == RR.REFKF_BOW_FAILED), tag
        if status == RR.REFKF_OK:
            for a, b in zip(lit["after_associate"], rk["after_associate"]):
                assert np.array_equal(a, b), tag
            assert lit["n_edges"] == rk["n_edges"][0] == rk["n_edges"][1] and np.array_equal(lit["edges"], rk["edges"]), tag
            assert lit["pose"]["Tcw_d"].tobytes() == rk["pose"]["Tcw_d"].tobytes() and lit["ret"] == rk["result"]["n_matches_map_refkf"][0], tag
    if status != RR.REFKF_OK:
        assert rk["n_edges"][1] == 0 and rk["pose"]["status"] == 1 and rk["result"]["n_matches_map_refkf"][0] == 0, tag
        assert np.array_equal(np.asarray(rk["pose"]["Tcw"], np.float32).reshape(4, 4), c["Tcw_last"]), tag
    assert (init["n_init"], init["success"]) == (rk["result"]["n_init"][0], rk["result"]["success"][0]), tag
    assert init["Tcw"].tobytes() == rk["Tcw_init"].tobytes(), tag
    for a, b in zip(init["state"], rk["state"]):
        assert np.array_equal(a, b), tag
    for a, b in zip(llocal["state"], local["state"]):
        assert np.array_equal(a, b), tag
    assert llocal["n_inliers"] == local["n_inliers"] and llocal["pose"]["Tcw_d"].tobytes() == local["pose"]["Tcw_d"].tobytes(), tag


@pytest.mark.parametrize("name", list(RC.DIRECTED))
def test_directed_cases_hold_and_literal_equals_dense(name):
    c, vv, ref = RC.directed(name)                                      # asserts the directed property and the qualification
    check_literal_equals_dense(c, vv, ref, name)


def test_random_cases_qualify_and_literal_equals_dense():
    cases, drawn = RC.random_cases()
    assert len(cases) == RC.N_RANDOM and 4 * len(cases) >= 3 * drawn      # at least three quarters of the seeds drawn qualify
    seen = set()
    for c, vv, ref in cases:
        check_literal_equals_dense(c, vv, ref, c["seed"])
        seen.add((vv, int(ref[1]["result"]["refkf_status"][0])))
    assert {(0, RR.REFKF_OK), (1, RR.REFKF_OK), (1, RR.REFKF_SKIPPED)} <= seen, seen


def test_shapes_are_the_smallest_that_reach_every_branch():
    c, _, (_, rk, _) = RC.directed("plain")
    K = c["K"]
    assert len(c["frame"]["kps"]) == 96 and len(c["lms"]) == 160 and K["n_kf"] == 3 and K["kf_off"][2] - K["kf_off"][1] == 80
    nodes = rk["bow_node"][rk["bow_weight"] > 0]
    assert len(np.unique(nodes)) <= 3 and np.bincount(np.unique(nodes, return_inverse=True)[1]).max() > 10      # several views share a node
    assert (rk["bow_weight"] <= 0).any() and (K["node"] < 0).any()                                                # words without weight on both sides
