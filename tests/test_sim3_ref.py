"""The reference of the batched Horn Sim3 RANSAC pinned by itself, on the CPU (tests/ref_sim3.py, tests/sim3_cases.py): the
plan's known answers, the sampler with its quirks, the closed form of the acceptance against the loop as written EXHAUSTIVELY, D19's rotation against
LITERAL's (atan2, angle-axis, Rodrigues) and against INDEPENDENT (Umeyama by SVD), the cases' qualification (asserted for every case, never a
filter), and the hand-derived answers of the directed cases."""
import itertools

import numpy as np

import ref_sim3 as R
import sim3_cases as SC
from hyslam_amd.synth import splitmix64

ULP1 = 2.0 ** -23


def test_plan_known_answers():
    its, eps = R.plan(100, 0.99, 20, 300)
    assert eps == np.float32(0.2) and its == 300
    assert R.plan(100, 0.99, 20, 10 ** 6)[0] == 574                # ceil(573.3...), uncapped
    assert R.plan(20, 0.99, 20, 300)[0] == 1                       # minInliers == N
    assert R.plan(40, 0.99, 20, 300)[0] == 35                      # epsilon 0.5: ceil(34.49)
    assert R.plan(100, 0.99, 20, 0)[0] == 1 and R.plan(100, 0.99, 20, -7)[0] == 1
    assert R.plan(100, 0.99, 0, 300)[0] == 1                       # log(1 - 0) = 0: the quotient is -inf
    assert R.plan(0, 0.99, 20, 300)[0] == 1 and R.plan(10, 0.99, 20, 300)[0] == 1      # epsilon inf / 2: log of a negative number
    assert R.plan(100, 1.0, 20, 300)[0] == 300                     # log(0) = -inf over a negative number: +inf, capped
    assert R.plan(100, 1.5, 20, 300)[0] == 1


def three_places(N, words):
    """the sampler as the kernel keeps it: only the places a draw wrote differ from their index"""
    pos, val, avail, out = [], [], N, []
    for k in range(3):
        randi, back = (int(words[k]) * avail) >> 32, avail - 1
        idx, at_b = randi, back
        for m in range(len(pos)):
            if pos[m] == randi:
                idx = val[m]
            if pos[m] == back:
                at_b = val[m]
        out.append(idx)
        if idx < avail:
            if idx in pos:
                val[pos.index(idx)] = at_b
            else:
                pos.append(idx)
                val.append(at_b)
        avail -= 1
    return out


def test_sampler_quirks_and_the_three_place_model():
    N = 12
    w = lambda places, n=N: [SC.word(p, n - k) for k, p in enumerate(places)]
    assert R.sample(N, w((3, 7, 1))) == [3, 7, 1]
    assert R.sample(N, w((0, 0, 9))) == [0, 11, 9]                 # a repeated place; the second write lands on a popped place: no effect
    assert R.sample(N, w((5, 5, 5))) == [5, 11, 11]                # the same point twice
    assert R.sample(N, w((11, 10, 9))) == [11, 10, 9]              # the back itself
    assert R.sample(N, w((2, 10, 2))) == [2, 10, 11]               # avail[2] = 11 after the first draw: the place drawn again gives 11
    assert R.sample(3, w((0, 0, 0), 3)) == [0, 2, 2]
    assert R.sample(N, [0xFFFFFFFF] * 3) == [11, 10, 9] and R.sample(N, [0, 0, 0]) == [0, 11, 11]
    for n in range(3, 8):                                          # every triple of places
        for places in itertools.product(range(n), range(n - 1), range(n - 2)):
            words = w(places, n)
            assert [(int(x) * (n - k)) >> 32 for k, x in enumerate(words)] == list(places)
            assert three_places(n, words) == R.sample(n, words), (n, places)


def test_generator_is_the_splitmix_sequence():
    seq = splitmix64(0, 64, 0) if splitmix64(0, 1, 0)[0] == R.mix(0) else None
    assert seq is not None, "hyslam_amd.synth.splitmix64(0, .) is the sequence D18 names"
    for seed, it, k in ((0, 0, 0), (5, 3, 2), (1, 20, 0)):
        assert R.draw32(seed, it, k) == int(seq[seed + 3 * it + k]) >> 32
    tab = np.array([[7, 8, 9, 0]], np.uint32)
    assert R.draw32(5, 0, 1, tab) == 8 and R.draw32(5, 1, 1, tab) == R.mix(5 + 3 + 1) >> 32


def test_closed_form_equals_the_loop_exhaustively():
    n = 0
    for length in range(0, 6):
        for counts in itertools.product(range(4), repeat=length):
            for best0 in range(4):
                for min_inliers in range(4):
                    assert R.closed_form(counts, best0, min_inliers) == R.loop_form(counts, best0, min_inliers), (counts, best0, min_inliers)
                    n += 1
    assert n == 16 * sum(4 ** k for k in range(6))


def test_solver_loop_and_closed_form_agree_on_every_case():
    for name, cs in SC.cases().items():
        a, b = SC.solver(cs), SC.solver(cs)
        for n in cs["calls"]:
            ra, rb = a.iterate(n), b.iterate_loop(n)
            for key in ("status", "n_inliers", "at_iteration", "iterations", "hypotheses_run"):
                assert ra[key] == rb[key], (name, key)
            for key in ("T12", "R", "t", "s", "mask"):
                assert np.array_equal(ra[key], rb[key], equal_nan=True), (name, key)
            assert (a.iterations, a.best_inliers) == (b.iterations, b.best_inliers) and np.array_equal(a.best_mask, b.best_mask), name


def _samples(cs):
    s = SC.solver(cs)
    if s.N < 3 or s.N < s.min_inliers:
        return None
    n = min(s.max_its, sum(cs["calls"]))
    idx = np.array(s.hypotheses(0, n)[0], np.int64)
    return cs["corrs"]["X1c"][idx], cs["corrs"]["X2c"][idx]


def test_d19_rotation_against_literal_within_one_float_ulp():
    worst, n = 0.0, 0
    for name, cs in SC.cases().items():
        xs = _samples(cs)
        if xs is None:
            continue
        N4 = R.horn_matrix(*xs)[4]
        quat = R.jacobi_quaternion(N4)
        d19, lit = R.quaternion_rotation(quat), R.literal_rotation(N4)
        for h in range(len(N4)):
            val = np.linalg.eigvalsh(N4[h].astype(np.float64))
            if name in SC.EXEMPT and not (np.isfinite(d19[h]).all() and val[3] - val[2] > 1e-6 * max(1.0, abs(val[3]))):
                assert name in ("identical_sets", "collinear_sample", "duplicate_sample"), name       # degenerate by construction
                if name == "identical_sets":
                    assert not np.isfinite(d19[h]).any() and not np.isfinite(lit[h]).any()                # 0 / 0 in both
                continue
            a, b = d19[h].astype(np.float32), lit[h].astype(np.float32)
            assert np.isfinite(a).all() and np.isfinite(b).all(), (name, h)
            worst = max(worst, float(np.abs(a.astype(np.float64) - b).max()))
            assert np.abs(a.astype(np.float64) - b).max() <= ULP1, (name, h)
            assert abs(np.linalg.norm(quat[h]) - 1) < 1e-14 and np.abs(d19[h] @ d19[h].T - np.eye(3)).max() < 1e-14, (name, h)
            n += 1
    print("D19 R against LITERAL: largest difference %.3g over %d hypotheses (bound %.3g)" % (worst, n, ULP1))
    assert n > 300


def test_pose_against_independent_umeyama():
    """float64 SVD against the float pipeline: the inputs are float32 and the centroid and relative coordinates are rounded to float32 (2^-24 relative
    of coordinates up to 9: 5e-7 absolute), which a sample whose smallest spread is sigma turns into a rotation error of about 5e-7 / sigma.  Samples
    with sigma >= 0.05 are held to 1e-4 (10 x that figure at the gate); the others are degenerate for any method."""
    n = 0
    for name, cs in SC.cases().items():
        xs = _samples(cs)
        if xs is None or name in SC.EXEMPT:
            continue
        Rm, t, s, _, _ = R.solve(xs[0], xs[1], cs["params"]["fix_scale"])
        for h in range(len(Rm)):
            B = xs[1][h].astype(np.float64)
            if np.linalg.svd(B - B.mean(0), compute_uv=False)[1] < 0.05:
                continue
            si, Ri, ti = R.umeyama(xs[0][h], xs[1][h], cs["params"]["fix_scale"])
            assert np.abs(Rm[h] - Ri).max() < 1e-4 and abs(s[h] - si) < 1e-4 * si and np.abs(t[h] - ti).max() < 1e-3, (name, h)
            n += 1
    assert n > 200


def test_qualification_holds_for_every_case():
    worst_rounding = max(SC.rounding(cs) for cs in SC.cases().values())
    print("float err against float64 err at LITERAL's poses, pairs below %g: largest difference %.3g; MARGIN %.3g" % (SC.NEAR, worst_rounding, SC.MARGIN))
    assert SC.MARGIN >= 8 * worst_rounding
    assert set(SC.EXEMPT) <= set(SC.cases())
    left_out = 0
    for name, cs in SC.cases().items():
        if name in SC.EXEMPT:
            continue
        q = SC.qualify(cs)
        print("%-24s smallest |err - threshold| %.4g" % (name, q))
        assert q > SC.MARGIN, (name, q)
        # what the margin buys: LITERAL's rotation decides every inlier as D19's does
        ab, ab_l = SC.all_hypotheses(cs), SC.all_hypotheses(cs, rotation="literal")
        if ab is not None:
            k1, k2 = np.asarray(cs["k1"], np.float32), np.asarray(cs["k2"], np.float32)
            assert np.array_equal(R.inliers(ab[0], ab[1], cs["corrs"], k1, k2), R.inliers(ab_l[0], ab_l[1], cs["corrs"], k1, k2)), name
    assert left_out == 0


def test_thresholds_truncate():
    th = R.threshold(np.array([1.0, 1.44, 2.0736, 2.985984, 0.0, -1.0, np.nan, np.inf, 1e30, 0.1], np.float32))
    assert th.tolist() == [9.0, 13.0, 19.0, 27.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert R.threshold(np.float32(2.0e18))[0] == np.float32(int(9.210 * float(np.float32(2.0e18))))      # below 2^64: converted, not refused


def test_directed_cases_hand_derived():
    C = SC.cases()
    res = {name: SC.run(cs) for name, cs in C.items()}
    st = lambda name: [r["status"] for r in res[name][0]]
    assert st("too_few") == [R.TOO_FEW] and st("n2_min0") == [R.TOO_FEW] and st("n0") == [R.TOO_FEW]
    assert res["too_few"][1].iterations == 0 and res["too_few"][1].best is None                    # the state is untouched
    assert st("n3_min3") == [R.EXHAUSTED] and res["n3_min3"][1].best_inliers == 3                  # 3 > 3 fails; one iteration
    assert st("n3_min2") == [R.FOUND] and st("n3_min0") == [R.FOUND]
    assert st("n_equals_min") == [R.EXHAUSTED, R.EXHAUSTED] and res["n_equals_min"][1].max_its == 1
    assert [r["hypotheses_run"] for r in res["n_equals_min"][0]] == [1, 0]                          # a call on an exhausted state runs none
    assert [r["hypotheses_run"] for r in res["exhausted_state"][0]] == [4, 0, 0] and st("exhausted_state") == [R.EXHAUSTED] * 3
    # equal counts: the last one is the best; a count equal to min_inliers does not return
    s = SC.solver(C["equal_counts_last_wins"])
    _, Rm, _, _, _, _, masks = s.hypotheses(0, 3)
    assert [int(m.sum()) for m in masks] == [8, 8, 8] and st("equal_counts_last_wins") == [R.CONTINUE]
    best = res["equal_counts_last_wins"][1].best
    assert np.array_equal(best[0], Rm[2]) and not np.array_equal(Rm[2], Rm[0]) and not np.array_equal(Rm[2], Rm[1])
    assert st("count_equals_min") == [R.CONTINUE, R.CONTINUE] and res["count_equals_min"][1].best_inliers == 8
    # three calls of 5 are one call of 15
    one = SC.solver(C["n100_rounds"])
    r15 = one.iterate(15)
    three = res["n100_rounds"][1]
    assert (one.iterations, one.best_inliers) == (three.iterations, three.best_inliers) and np.array_equal(one.best_mask, three.best_mask)
    assert r15["status"] == res["n100_rounds"][0][-1]["status"]
    # thresholds
    for name, lo, hi in (("sigma_1_44", 13.0, 13.26), ("err_equals_threshold", 13.0, 13.0)):
        s = SC.solver(C[name])
        _, _, _, _, a, b, masks = s.hypotheses(0, 1)
        e1, e2 = R.errors(a, b, C[name]["corrs"], s.k1, s.k2)
        assert lo <= e1[0, 9] <= hi and (name != "sigma_1_44" or e1[0, 9] > 13.0) and e2[0, 9] < 13.0 and masks[0].tolist() == [True] * 9 + [False], (name, e1[0, 9])
    # depth: z = 0 is an outlier on either side, a consistent point behind the cameras is an inlier
    assert res["z_zero_or_negative"][0][0]["mask"].tolist() == [1] * 13 + [0, 0, 1]
    s = SC.solver(C["z_zero_or_negative"])
    assert [int(m.sum()) for m in s.hypotheses(0, 4)[6]] == [14, 0, 0, 14]                           # a sample with a z = 0 point; one with the point behind
    # identical point sets: every hypothesis is non-finite and counts nothing; 0 >= 0 makes it the best all the same
    r, s = res["identical_sets"]
    assert r[0]["status"] == R.EXHAUSTED and s.best_inliers == 0 and not np.isfinite(s.best[0]).any() and not s.best_mask.any()
    # a duplicated point: a rank-one sample
    assert R.sample(12, C["duplicate_sample"]["draws"][0]) == [5, 11, 11] and R.sample(12, C["popped_slot"]["draws"][0]) == [0, 11, 9]
    assert st("popped_slot") == [R.FOUND] and res["popped_slot"][0][0]["n_inliers"] == 12
    assert st("n100") == [R.FOUND] and res["n100"][0][0]["at_iteration"] == res["n100"][1].iterations == 2
