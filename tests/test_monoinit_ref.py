"""CPU: pins the reference of the monocular initialisation (tests/ref_monoinit.py) before anything is compared with it: Normalize, ComputeH21 and
ComputeF21 on exact data, the rank-2 property of F, the sampler against the Python twin of hs_ransac_sample, the decision rules on hand-made
tuples, LITERAL against INDEPENDENT, and the qualification of the cases of tests/monoinit_cases.py.

TOLERANCE.  LITERAL and INDEPENDENT share no decomposition; both work in float64 on the same float32 operands and narrow once, so they can differ
where a float64 result falls within about 1e-15 relative of a float32 rounding boundary, and then by one unit in the last place of the float32
(2^-24 relative to a unit-norm model).  MEASURED over every hypothesis of every non-exempt case and sweep scene (the test prints the figure): 3.3e-15 for the models
(unit norm, sign aligned; 0.0 with another numpy build) and 0.0 relative for the scores.  The assert allows 4 x max(measured, 2^-24): the measured
figure is far below the number format's one rounding, so that rounding is the bound; the factor is headroom for another libm or numpy build, not for the code
under test.  A score is a sum of up to 2 N terms of magnitude below 6, so its bound is relative to max(1, score) and 2 N times the model's."""
import numpy as np
import pytest

import monoinit_cases as MC
import ref_monoinit as R
import ref_pnp

F32 = np.float32
MEASURED_MODEL, MEASURED_SCORE = 3.3e-15, 0.0
TOL_MODEL = 4 * max(MEASURED_MODEL, 2.0 ** -24)


def everything():
    out = dict(MC.cases())
    out.update(MC.sweep())
    return out


def qualified():
    return [n for n in sorted(everything()) if n not in MC.EXEMPT and n not in SWEEP_EXEMPT]


# sweep scenes that sit on an edge by chance (at most 4 of 32), compared with LITERAL only.  With SWEEP_SEED = 9000: sweep11 has N = 8 (equal scores,
# the first wins), sweep25 has nGood = 25 and 17, half a point from 0.7 x 25.
SWEEP_EXEMPT = ("sweep11", "sweep25")


def test_normalize():
    xy = (MC.uniform(3, 200, 1).reshape(100, 2) * 600).astype(F32)
    pn, T, (mx, my, sx, sy) = R.normalize(xy)
    assert abs(float(pn[:, 0].mean())) < 1e-5 and abs(float(pn[:, 1].mean())) < 1e-5
    assert abs(float(np.abs(pn[:, 0]).mean()) - 1) < 1e-5 and abs(float(np.abs(pn[:, 1]).mean()) - 1) < 1e-5
    h = np.concatenate([xy, np.ones((100, 1), F32)], 1).astype(np.float64) @ T.astype(np.float64).T
    assert np.allclose(h[:, :2], pn, atol=1e-4) and T[2].tolist() == [0, 0, 1] and T[0, 1] == 0 and T[1, 0] == 0
    # the sums run in key order in float32: the mean is the sequential one, not numpy's pairwise one
    seq = F32(0)
    for v in xy[:, 0]:
        seq = F32(seq + v)
    assert mx == F32(seq / F32(100))


def exact_two_views(seed, plane):
    N = 8
    u, v = (MC.uniform(seed, N, 1) - 0.5), (MC.uniform(seed, N, 2) - 0.5) * 0.75
    z = 5.0 / (1.0 - 0.16 * u - 0.1 * v) if plane else 3.0 + 6.0 * MC.uniform(seed, N, 3)
    X = np.stack([u * z, v * z, z], 1)
    Rm, t = MC.rotation(seed, 0.2), np.array([0.4, 0.05, 0.1])
    X2 = X @ Rm.T + t
    return X, X2, Rm, t


@pytest.mark.parametrize("la", [R.Literal, R.Independent])
def test_compute_h21_recovers_the_homography_of_a_plane(la):
    X, X2, Rm, t = exact_two_views(5, True)
    p1, p2 = (X[:, :2] / X[:, 2:]), (X2[:, :2] / X2[:, 2:])
    H = R.compute_h21(p1.astype(F32)[None], p2.astype(F32)[None], la)[0].astype(np.float64)
    q = np.concatenate([p1, np.ones((8, 1))], 1) @ H.T
    assert np.abs(q[:, :2] / q[:, 2:] - p2).max() < 1e-4
    k = np.argmax(np.abs(H.reshape(-1)))
    assert H.reshape(-1)[k] > 0                                    # D20's orientation


@pytest.mark.parametrize("la", [R.Literal, R.Independent])
def test_compute_f21_recovers_the_epipolar_geometry_and_has_rank_two(la):
    X, X2, Rm, t = exact_two_views(6, False)
    p1, p2 = (X[:, :2] / X[:, 2:]), (X2[:, :2] / X2[:, 2:])
    F = R.compute_f21(p1.astype(F32)[None], p2.astype(F32)[None], la)[0].astype(np.float64)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ Rm
    a, b = F / np.linalg.norm(F), E / np.linalg.norm(E)
    assert min(np.abs(a - b).max(), np.abs(a + b).max()) < 1e-3
    s = np.linalg.svd(F)[1]
    assert s[2] < 1e-6 * s[0] and s[1] > 1e-2 * s[0]


def test_sampler_is_the_swap_with_back_twin():
    """sample_sets is hs_ransac_sample<8, false>'s Python twin (ref_pnp.sample on D18's words): distinct indices in range, H and F share them, a
    directed table names the PLACES drawn, and the generator's words are SplitMix64 on the counter seed + 8 it + k"""
    for N in (8, 9, 40, 257):
        sets = R.sample_sets(N, 50, 12345)
        assert all(len(set(s)) == 8 and min(s) >= 0 and max(s) < N for s in sets)
    assert sorted(R.sample_sets(8, 1, 7)[0]) == list(range(8))
    d = MC.table([[0, 0, 0, 0, 0, 0, 0, 0], [39, 38, 37, 36, 35, 34, 33, 32]], 40)
    sets = R.sample_sets(40, 3, 99, d)
    assert sets[0] == [0, 39, 38, 37, 36, 35, 34, 33] and sets[1] == [39, 38, 37, 36, 35, 34, 33, 32]
    assert sets[2] == ref_pnp.sample(40, 8, [ref_pnp.mix(99 + 16 + k) >> 32 for k in range(8)])
    from hyslam_amd.features import _ransac_words
    w = _ransac_words(99, 3, 8, 8)
    assert [int(x) for x in w[2]] == [ref_pnp.mix(99 + 16 + k) >> 32 for k in range(8)]


def test_decision_rules_on_hand_made_tuples():
    T, F_ = True, False
    ok8 = [T] * 8
    # ReconstructF: nMinGood = max((int)(0.9 N), minTri); nsimilar counts > 0.7 maxGood; the first motion equal to the maximum decides alone
    assert R.decide_f([100, 0, 0, 0], ok8, 100, 50, 0.9) == (0, 0)
    assert R.decide_f([0, 0, 100, 10], ok8, 100, 50, 0.9) == (2, 2)
    assert R.decide_f([100, 71, 0, 0], ok8, 100, 50, 0.9) == (-1, -1)              # 71 > 70: two similar
    assert R.decide_f([100, 70, 0, 0], ok8, 100, 50, 0.9) == (0, 0)                # 70 > 70.0 is false
    assert R.decide_f([89, 0, 0, 0], ok8, 100, 50, 0.9) == (-1, -1)                # below (int)(0.9 * 100) = 90
    assert R.decide_f([90, 0, 0, 0], ok8, 100, 50, 0.9) == (0, 0)
    assert R.decide_f([40, 0, 0, 0], ok8, 40, 50, 0.9) == (-1, -1)                 # below minTriangulated
    assert R.decide_f([0, 60, 0, 60], [T, F_, T, T, T, T, T, T], 60, 50, 0.9) == (-1, -1)       # a tie is two similar
    assert R.decide_f([0, 60, 0, 0], [T, F_, T, T, T, T, T, T], 60, 50, 0.9) == (-1, 1)         # the decider lacks parallax: nobody else is asked
    assert R.decide_f([0, 0, 0, 0], [F_] * 8, 0, 0, 0.9) == (-1, 0)                # maxGood = 0 passes both gates; parallax 0 fails
    # ReconstructH: second < 0.75 best, best > minTri, best > frac N, parallax >=
    assert R.decide_h([10, 100, 74, 0, 0, 0, 0, 0], ok8, 100, 50, 0.9) == (1, 1)
    assert R.decide_h([10, 100, 75, 0, 0, 0, 0, 0], ok8, 100, 50, 0.9) == (-1, 1)  # 75 < 75.0 is false
    assert R.decide_h([100, 100, 0, 0, 0, 0, 0, 0], ok8, 100, 50, 0.9) == (-1, 0)  # the second 100 is not > best: it becomes the second best
    assert R.decide_h([50, 0, 0, 0, 0, 0, 0, 0], ok8, 50, 50, 0.9) == (-1, 0)      # best > minTri is strict
    assert R.decide_h([90, 0, 0, 0, 0, 0, 0, 0], ok8, 100, 50, 0.9) == (-1, 0)     # best > 0.9f * 100 is strict
    assert R.decide_h([91, 0, 0, 0, 0, 0, 0, 0], ok8, 100, 50, 0.9) == (0, 0)
    assert R.decide_h([91, 0, 0, 0, 0, 0, 0, 0], [F_] + [T] * 7, 100, 50, 0.9) == (-1, 0)
    assert R.decide_h([0] * 8, ok8, 100, 50, 0.9) == (-1, -1)
    # the rank of the parallax is minTriangulated, not a median (quirk 5)
    c = np.array([0.5, 0.1, 0.9, 0.3], F32)
    assert R.selected_cosine(c, 1) == F32(0.3) and R.selected_cosine(c, 50) == F32(0.9) and R.selected_cosine(c, 0) == F32(0.1)
    # D21's constant
    assert R.cos_min_parallax(1.0) == F32(0.9998477) and R.cos_min_parallax(1.0) > F32(0.99984)


def _unit(M):
    M = M.reshape(len(M), -1).astype(np.float64)
    return M / np.linalg.norm(M, axis=1, keepdims=True)


def test_expected_outcomes_and_literal_against_independent():
    worst_model = worst_score = 0.0
    for name in qualified():
        c = everything()[name]
        a, b = MC.run_reference(c), MC.run_reference(c, "independent")
        if c["expect"] is not None:
            assert a["status"] == c["expect"], (name, a["status"])
        hyp, hyq = a["hyp"], b["hyp"]
        N = a["n_matches"]
        for mk, sk in (("H21", "score_h"), ("F21", "score_f")):
            ua, ub = _unit(hyp[mk]), _unit(hyq[mk])
            sgn = np.sign((ua * ub).sum(1, keepdims=True))
            d = np.abs(ua - sgn * ub).max(1)
            assert np.isfinite(d).all(), (name, mk, "a non-finite model in a qualified case")
            worst_model = max(worst_model, float(d.max()))
            sa, sb = hyp[sk].astype(np.float64), hyq[sk].astype(np.float64)
            ds = float((np.abs(sa - sb) / np.maximum(1.0, np.abs(sa))).max())
            worst_score = max(worst_score, ds)
            assert d.max() <= TOL_MODEL and ds <= 2 * N * TOL_MODEL, (name, mk, float(d.max()), ds)
        # winners, masks, decisions
        assert (a["status"], a["model"], a["best_it_h"], a["best_it_f"]) == (b["status"], b["model"], b["best_it_h"], b["best_it_f"]), name
        assert np.array_equal(a["inliers_h"], b["inliers_h"]) and np.array_equal(a["inliers_f"], b["inliers_f"]), name
        # the motions' order depends on the signs a decomposition gives its vectors: the counts are compared as a multiset, the pose as a pose
        assert sorted(a["n_good"]) == sorted(b["n_good"]) and a["n_triangulated"] == b["n_triangulated"], name
        assert np.array_equal(a["triangulated"], b["triangulated"]), name
        if a["status"] in (R.OK_H, R.OK_F):
            assert np.abs(a["R21"] - b["R21"]).max() < 1e-5 and np.abs(a["t21"] - b["t21"]).max() < 1e-5, name
            tri = a["triangulated"] != 0
            assert np.abs(a["p3d"][tri] - b["p3d"][tri]).max() < 1e-3 * np.abs(a["p3d"][tri]).max(), name
            assert abs(float(a["cos_parallax"]) - float(b["cos_parallax"])) < 1e-6, name
    print("LITERAL against INDEPENDENT: largest model deviation %.3e (allowed %.3e), largest relative score deviation %.3e" % (worst_model, TOL_MODEL, worst_score))


def test_qualification_of_the_cases():
    """asserted with the reference alone: every chi-square of every hypothesis at least 1e-4 relative from its threshold, the best score's lead over the
    runner-up above the tolerance, the selected cosine at least 1e-6 relative from D21's constant, the nGood ratios away from 0.7 / 0.75"""
    assert len(SWEEP_EXEMPT) <= 4 and all(n in MC.sweep() for n in SWEEP_EXEMPT)
    for name in qualified():
        c = everything()[name]
        a = MC.run_reference(c)
        hyp, N = a["hyp"], a["n_matches"]
        ch1, ch2, cf1, cf2 = hyp["chi"]
        for chis, th in (((ch1, ch2), 5.991), ((cf1, cf2), 3.841)):        # EVERY chi-square of every hypothesis: every score is compared
            for ch in chis:
                x = ch.astype(np.float64)
                x = x[np.isfinite(x)]
                assert (np.abs(x - th) >= 1e-4 * th).all(), (name, "a chi-square on its threshold", th, float(np.abs(x - th).min()))
        for sk in ("score_h", "score_f"):
            s = np.sort(hyp[sk].astype(np.float64))[::-1]
            if len(s) > 1 and s[0] > 0:
                assert s[0] - s[1] > 2 * N * TOL_MODEL * max(1.0, s[0]) or s[0] == s[1] == 0, (name, sk, "the best score's lead", s[0] - s[1])
        cmin = float(R.cos_min_parallax(c["params"]["min_parallax_deg"]))
        if a["best_solution"] >= 0 and a["n_good"][a["best_solution"]] > 0:
            assert abs(float(a["cos_parallax"]) - cmin) >= 1e-6 * cmin, (name, "the selected cosine on D21's constant")
        g = sorted((int(x) for x in a["n_good"]), reverse=True)
        if g[0] > 0:
            for x in g[1:]:
                assert abs(x - 0.7 * g[0]) > 0.5 and abs(x - 0.75 * g[0]) > 0.5 or x == 0, (name, "an nGood ratio on 0.7 / 0.75", g)


def test_exempt_cases_do_what_they_were_built_for():
    c = MC.cases()
    a = MC.run_reference(c["identical_points"])
    assert a["status"] == R.FAILED and a["best_it_h"] == -1 and a["best_it_f"] == -1 and not np.isfinite(a["hyp"]["score_h"]).any()       # a NaN never wins
    a = MC.run_reference(c["both_scores_zero"])
    assert a["n_matches"] == 9 and a["score_h"] == 0 and a["score_f"] == 0 and np.isnan(a["rh"]) and a["model"] == R.MODEL_NONE and a["status"] == R.FAILED
    assert not a["inliers_f"].any()                                # quirk 2
    a = MC.run_reference(c["n7_too_few"])
    assert a["status"] == R.TOO_FEW and a["n_matches"] == 7 and a["hyp"] is None
    a = MC.run_reference(c["two_motions_tie"])
    g = sorted((int(x) for x in a["n_good"]), reverse=True)
    assert a["model"] == R.MODEL_H and a["status"] == R.FAILED and g[1] >= 0.75 * g[0] > 0      # the 0.75 rule
    a = MC.run_reference(c["pure_rotation"])
    assert a["status"] == R.FAILED and a["model"] == R.MODEL_H and not a["n_good"].any()
    a, b = MC.run_reference(c["min_tri_above_accepted"]), MC.run_reference(c["min_tri_below_accepted"])
    assert a["n_good"].max() == b["n_good"].max() == 60 and (a["status"], b["status"]) == (R.FAILED, R.OK_F)      # both branches of the rank ran: 500 > 59 >= 10
    shapes = {n: (len(c[n]["kps1"]), len(c[n]["kps2"]), MC.run_reference(c[n])["n_matches"]) for n in ("general_f", "key_chunk+0")}
    assert all(n1 != n2 and n1 > N and n2 > N for n1, n2, N in shapes.values())
