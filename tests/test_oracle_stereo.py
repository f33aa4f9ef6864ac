"""The oracle's stereo matcher (oracle/hs_oracle.cpp, computeStereoMatches) against the independent numpy restatement
pyref.stereo_match, on generated edge cases (scenes.stereo_edge_lists) and on hand-built ones whose answer is known."""
import os

import numpy as np
import pytest

import oracle
import pyref
import scenes

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def both(kL, dL, kR, dR, params):
    o = oracle.stereo_match(kL, dL, kR, dR, oracle.stereo_params(**params))
    p = pyref.stereo_match(kL, dL, kR, dR, **params)
    return o, p


def assert_same(o, p, what):
    ou, oz, obi, obd = o
    pu, pz, pbi, pbd = p
    bad = np.nonzero((ou.view(np.uint32) != pu.view(np.uint32)) | (oz.view(np.uint32) != pz.view(np.uint32)) | (obi != pbi) | (obd != pbd))[0]
    assert len(bad) == 0, "%s: %d keypoints differ, first iL=%d: oracle (uR %r, depth %r, best %d @ %d) pyref (uR %r, depth %r, best %d @ %d)" % (
        what, len(bad), bad[0], ou[bad[0]], oz[bad[0]], obd[bad[0]], obi[bad[0]], pu[bad[0]], pz[bad[0]], pbd[bad[0]], pbi[bad[0]])


@pytest.mark.parametrize("kind", scenes.STEREO_EDGE_KINDS)
def test_edge_cases_match_restatement(kind):
    rng = np.random.default_rng(sum(map(ord, kind)))
    matched = 0
    for case in range(40):
        kL, dL, kR, dR, params = scenes.stereo_edge_lists(rng, kind)
        o, p = both(kL, dL, kR, dR, params)
        assert_same(o, p, "%s case %d %r" % (kind, case, params))
        matched += int((o[1] > 0).sum())
    assert matched > 100, matched


@pytest.mark.parametrize("n_rows", [0, 1, 33, 480, 1080, 1087])
def test_parameter_grid(n_rows):
    """every n_rows against every band width (1, 2, 3 and more strips; r < 1) and threshold pair"""
    rng = np.random.default_rng(100 + n_rows)
    for size_ref in (31.0, 7.5, 4.0, 1e6):
        for th in scenes.STEREO_THRESHOLDS + ((80.0, 120.0),):
            kind = scenes.STEREO_EDGE_KINDS[int(rng.integers(len(scenes.STEREO_EDGE_KINDS)))]
            kL, dL, kR, dR, params = scenes.stereo_edge_lists(rng, kind, n_rows=n_rows, size_ref=size_ref, th=th)
            o, p = both(kL, dL, kR, dR, params)
            assert_same(o, p, repr(params))
            if n_rows == 0:
                assert (o[0] == -1).all() and (o[1] == -1).all()


def test_empty_and_single_lists():
    rng = np.random.default_rng(7)
    for nL, nR in ((0, 0), (0, 5), (1, 0), (1, 1), (5, 0), (1, 40), (40, 1)):
        for kind in ("mixed", "disparity", "ties"):
            kL, dL, kR, dR, params = scenes.stereo_edge_lists(rng, kind, nL=nL, nR=nR, n_rows=480)
            o, p = both(kL, dL, kR, dR, params)
            assert_same(o, p, "nL %d nR %d %s" % (nL, nR, kind))
            if nR == 0:
                assert (o[1] == -1).all()


@pytest.mark.parametrize("nL,nR", [(2049, 1500), (2900, 2900), (700, 2999)])
def test_larger_lists_match_restatement(nL, nR):
    rng = np.random.default_rng(nL + nR)
    for kind in ("mixed", "median", "boundaries"):
        kL, dL, kR, dR, params = scenes.stereo_edge_lists(rng, kind, nL=nL, nR=nR, n_rows=1080, size_ref=7.5 if kind == "boundaries" else 31.0)
        o, p = both(kL, dL, kR, dR, params)
        assert_same(o, p, "%s %d x %d" % (kind, nL, nR))
        assert (o[1] > 0).sum() > nL // 20


@pytest.mark.parametrize("n", [4097, 9000, 20000])
def test_large_lists_are_order_independent(n):
    """Beyond what the restatement runs: the oracle against itself.  Shuffling the left list permutes the results exactly (each left
    keypoint is matched on its own, the median cut only sees the multiset of distances).  Shuffling the right list keeps the best distance
    of every keypoint matched both times, and uRight/depth wherever the same right keypoint still wins (only equal distances can change
    the winner)."""
    rng = np.random.default_rng(n)
    kL, dL, kR, dR, params = scenes.stereo_edge_lists(rng, "mixed", nL=n, nR=n, n_rows=1087, size_ref=7.5, th=(100.0, 51.0), fx=1050.0)
    sp = oracle.stereo_params(**params)
    u, z, bi, bd = oracle.stereo_match(kL, dL, kR, dR, sp)
    assert (z > 0).sum() > n // 20
    pl = rng.permutation(n)
    u2, z2, bi2, bd2 = oracle.stereo_match(kL[pl], dL[pl], kR, dR, sp)
    assert np.array_equal(u2, u[pl]) and np.array_equal(z2, z[pl]) and np.array_equal(bi2, bi[pl]) and np.array_equal(bd2, bd[pl])
    pr = rng.permutation(n)
    u3, z3, bi3, bd3 = oracle.stereo_match(kL, dL, kR[pr], dR[pr], sp)
    both_matched = (bd >= 0) & (bd3 >= 0)         # a different winner among equal distances may sit at disparity == maxD and be rejected
    assert np.array_equal(bd3[both_matched], bd[both_matched]) and (bd3 >= 0).sum() > 0.99 * (bd >= 0).sum()
    same = (bi >= 0) & (bi3 >= 0)
    same[same] = pr[bi3[same]] == bi[same]
    assert same.sum() > n // 20
    assert np.array_equal(u3[same], u[same]) and np.array_equal(z3[same], z[same])


def test_committed_golden_pair():
    g = np.load(os.path.join(G, "stereo_640x480_1000.npz"))
    fx = float(g["fx"])
    u, z, bi, bd = pyref.stereo_match(g["kL"], g["dL"], g["kR"], g["dR"], fx=fx, mbf=fx * 0.12, n_rows=int(g["h"]), th_high=100.0, th_low=50.0, size_ref=31.0)
    assert np.array_equal(u, g["uRight"]) and np.array_equal(z, g["depth"])
    m = z > 0
    assert m.sum() > 200 and np.array_equal(bi[m], g["best_idx"][m]) and np.array_equal(bd[m], g["best_dist"][m])


# ---------------------------------------------------------------- hand-built cases with a known answer
def kps(*rows):
    k = np.zeros(len(rows), oracle.KP_DTYPE)
    for i, (x, y, octave) in enumerate(rows):
        k[i]["x"], k[i]["y"], k[i]["octave"] = x, y, octave
        k[i]["size"] = np.float32(31) * np.float32(1.2) ** np.float32(octave)
    return k


def run_known(kL, dL, kR, dR, **kw):
    params = dict(fx=500.0, mbf=60.0, n_rows=480, th_high=100.0, th_low=50.0, size_ref=31.0)
    params.update(kw)
    o, p = both(kL, dL, kR, dR, params)
    assert_same(o, p, repr(params))
    return o


def test_known_zero_disparity_and_window_edge():
    rng = np.random.default_rng(1)
    dL = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    f = np.float32
    max_d = f(f(60.0) / f(f(60.0) / f(500.0)))
    uL = f(700.0)
    assert f(uL - max_d) + max_d == uL                                       # uL - maxD is exact: disparity == maxD below
    kL = kps((uL, 100.0, 0), (uL, 200.0, 0), (uL, 300.0, 0))
    kR = kps((uL, 100.0, 0), (f(uL - max_d), 200.0, 0), (np.nextafter(uL, f(1e9)), 300.0, 0))
    u, z, bi, bd = run_known(kL, dL, kR, scenes.flip_bits(rng, dL, [4, 4, 4]), th_low=95.0)
    assert u[0] == f(np.float64(uL) - 0.01) and z[0] == f(60.0) / f(0.01)    # uR == uL: the 0.01 px clamp
    assert u[1] == -1 and bi[1] == -1                                        # disparity == maxD: in the window, rejected by `< maxD`
    assert u[2] == -1 and bi[2] == -1                                        # one ulp right of uL: outside the window


def test_known_equal_distances_lowest_index_wins():
    """three right keypoints at one distance whose row bands cover the left row from three different 32-row strips; in every list order
    the lowest index wins (the reference's strict `dist < bestDist` over ascending iR)"""
    rng = np.random.default_rng(2)
    dL = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    rows = [(600.0, 40.0, 0), (590.0, 71.0, 0), (580.0, 25.0, 0)]                # size 31, size_ref 2: r = 31 rows; strips 1, 2, 0
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        kR = kps(*[rows[i] for i in order])
        dR = scenes.flip_bits(rng, np.repeat(dL, 3, 0), 7)
        u, z, bi, bd = run_known(kps((620.0, 55.5, 0)), dL, kR, dR, size_ref=2.0)
        assert bi[0] == 0 and bd[0] == 7 and u[0] == rows[order[0]][0], order


def test_known_band_edges():
    """size 31, size_ref 7.5: r = 8.2667 rows; the band of y = 40.5 is rows floor(32.23) .. ceil(48.77) = 32 .. 49"""
    rng = np.random.default_rng(3)
    ys = [31.999, 32.0, 49.0, 49.999, 50.0]
    dL = rng.integers(0, 256, (len(ys), 32), dtype=np.uint8)
    u, z, bi, bd = run_known(kps(*[(500.0, y, 0) for y in ys]), dL, kps(*[(450.0, 40.5, 0)] * len(ys)), dL, size_ref=7.5, th_low=90.0)
    assert (bi == [-1, 1, 2, 3, -1]).all()                                   # rows 31 and 50 lie outside the band


def test_known_median_cut():
    """median of the sorted distances is element size // 2; distances >= 2.1 * median are cut (sorted 2 3 10 11 21 24: median 11,
    only 24 is cut; element 2 would cut 21 too)"""
    rng = np.random.default_rng(4)
    dists = [11, 24, 2, 21, 10, 3]
    n = len(dists)
    dL = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    kL = kps(*[(500.0, 10.0 + 40 * i, 0) for i in range(n)])
    kR = kps(*[(450.0, 10.0 + 40 * i, 0) for i in range(n)])
    u, z, bi, bd = run_known(kL, dL, kR, scenes.flip_bits(rng, dL, dists))
    assert (bd == dists).all() and list(u > 0) == [True, False, True, True, True, True]


def test_known_no_candidate_below_th_high_with_th_low_above():
    """Regression: a left keypoint whose row has candidates but none under TH_HIGH keeps the reference's initial bestDist = TH_HIGH and
    bestIdxR = 0 (Stereomatcher.cpp:92-93).  With TH_LOW > TH_HIGH that passes `bestDist < (TH_HIGH + TH_LOW) / 2`, so the keypoint is
    paired with right keypoint 0, even though keypoint 0 is in another row and another octave."""
    rng = np.random.default_rng(5)
    dL = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    kL = kps((500.0, 100.0, 0), (500.0, 300.0, 0))
    kR = kps((470.0, 10.0, 5), (490.0, 100.0, 0))
    dR = np.stack([rng.integers(0, 256, 32, dtype=np.uint8), scenes.flip_bits(rng, dL[:1], 90)[0]])
    u, z, bi, bd = run_known(kL, dL, kR, dR, th_high=80.0, th_low=120.0)
    assert bi[0] == 0 and bd[0] == 80 and u[0] == np.float32(470.0)        # distance 90 >= TH_HIGH: the initial values stand
    assert bi[1] == -1                                                       # row 300 has no candidate: skipped before the search
