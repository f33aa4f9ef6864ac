"""CPU: the runs of tests/chain_run.py resolve and have the properties tests/test_gpu_chain_run.py relies on: every slot's property in the reference,
sizes that cross the wave (64), the workgroup (256) and the 1024-landmark block in both directions, frames that insert a key frame and frames that do
not, a frame that creates fewer landmarks than it has room for, slot H built from the reference's result of G, slot I the object of slot A."""
import numpy as np

import chain_run as CR
import ref_track as R


def test_every_slot_resolves_with_its_property():
    fr = CR.run()
    assert sorted(fr) == sorted(CR.SLOTS)
    for slot in "ABCDEFGH":
        f = fr[slot]
        assert CR.PROPERTY[slot](*f.ref), slot
        assert (f.kf is not None) == (f.ref[0]["status"] == R.TRACK_OK), slot
    a, b, e, g = fr["A"], fr["B"], fr["E"], fr["G"]
    assert (a.n, a.n_last, a.L) == (300, 200, 400) and (g.n, g.n_last, g.L, g.c["frame"]["sensor"]) == (257, 130, 320, 0)
    assert (e.n, e.L) == (1025, 1225) and fr["D"].kf is None and fr["F"].ref[0]["n_edges"] < 3
    assert b.n == CR.B_N <= 64 and b.n_last < b.n and b.L < 128


def test_slot_b_is_the_smallest():
    # below 30 views the last frame has fewer than n_min_matches = 20 keypoints and the motion stage cannot succeed; the sizes from there on are tried
    assert CR.b_args(29)["n_last"] < R.TrackParams().n_min_matches <= CR.b_args(30)["n_last"]
    assert CR.smallest_b(lo=30) == CR.B_N


def test_sizes_cross_the_thresholds_both_ways():
    for order in CR.ORDERS:
        frames = CR.ordered(order)
        assert sorted(f.slot for f in frames) == sorted(fr.slot for fr in CR.run().values())
        pos = {f.slot: i for i, f in enumerate(frames)}
        assert pos["H"] == pos["G"] + 1, order
    frames = CR.ordered("table")
    for size, edges in ((lambda f: f.n, (64, 256, 1024)), (lambda f: f.L, (64, 256, 1024)), (lambda f: f.n_last, (64, 256))):
        v = [size(f) for f in frames]
        for t in edges:
            up = any(a <= t < b for a, b in zip(v, v[1:]))
            down = any(a > t >= b for a, b in zip(v, v[1:]))
            assert up and down, (v, t)
    # the buffers are never refilled, so what a frame finds in them is what ALL frames before it left: over the orders every case but the largest
    # runs somewhere after a larger frame, and every case but the smallest somewhere after a smaller one
    after_larger, after_smaller = set(), set()
    for order in CR.ORDERS:
        fs = CR.ordered(order)
        for i, f in enumerate(fs):
            if any(p.n > f.n for p in fs[:i]):
                after_larger.add(id(f))
            if any(p.n < f.n for p in fs[:i]):
                after_smaller.add(id(f))
    ns = [f.n for f in frames]
    for f in frames:
        assert f.n == max(ns) or id(f) in after_larger, f.slot
        assert f.n == min(ns) or id(f) in after_smaller, f.slot
    asc = CR.ordered("ascending")
    assert [f.n for f in asc[:-1]] == sorted(f.n for f in asc[:-1]) and asc[-1].n < asc[-2].n


def test_keyframe_outcomes():
    fr = CR.run()
    res = {s: CR.keyframe_reference(f)["result"] for s, f in fr.items() if f.kf is not None and s != "I"}
    assert sum(r["insert"] == 1 for r in res.values()) >= 2 and sum(r["insert"] == 0 for r in res.values()) >= 2
    assert any(0 < r["n_new"] < fr[s].new_cap for s, r in res.items()) and any(r["n_new"] == 0 for r in res.values())
    assert any(r["ok"] == 0 for r in res.values())                          # and one frame the gate closes on (stages 3-6 write zeros)
    assert all(fr[s].kf["insert"] == (r["insert"] == 1) for s, r in res.items() if r["ok"])


def test_slot_h_from_the_reference_of_g_and_slot_i_is_slot_a():
    fr = CR.run()
    g, h = fr["G"], fr["H"]
    kf = CR.keyframe_reference(g)
    c, ref, ok = CR.derive_h(g, kf["kp_lm"], g.ref[1]["pose"]["Tcw"])
    assert ok and np.array_equal(c["last_kp_lm"], h.c["last_kp_lm"]) and c["last_kps"] is g.c["frame"]["kps"] and h.c["frame"] is g.c["frame"]
    assert h.c["lms"] is g.c["lms"] and h.c["T"] is g.c["T"] and h.n_last == g.n
    assert fr["I"] is fr["A"] and CR.run() is fr


def test_refkf_run():
    frames = CR.refkf_run()
    assert [f["n"] for f in frames] == [130, 5, 1025, 64, 257]
    rel = [np.sign(f["kf_cap"] - f["nk"]) for f in frames]
    assert {-1, 0, 1} <= set(rel)
    for f in frames:
        match_kf, op_view, op_lm, nm = f["search"]
        assert nm > 0 and len(match_kf) == f["kf_cap"] and len(op_view) == f["n"]
        live = match_kf[match_kf >= 0]
        assert f["n"] < 64 or len(np.unique(live)) < len(live)              # two key-frame keypoints take one view
        assert not np.array_equal(f["state"][0], f["state0"][0])
