"""CPU: the reference of the batched EPnP RANSAC (tests/ref_pnp.py) pinned before the device is compared with it — known answers for the plan, the
sampler's swap-with-back rule, the closed "records" form of the loop against the loop as written (exhaustively), LITERAL against INDEPENDENT, and
the qualification of every case of tests/pnp_cases.py (asserted, never a filter).  Most of this file exercises tests/ref_pnp.py alone and passes
without the library's hs_pnp_* symbols; test_plan_of_the_library_is_the_reference_plan, tests/test_pnp_abi.py and the GPU files are the ones that need them."""
import itertools

import numpy as np
import pytest

import pnp_cases as PC
import ref_pnp as R

NAMES = sorted(PC.cases())


# ---------------------------------------------------------------- SetRansacParameters: answers derivable by hand
@pytest.mark.parametrize("N, over, want", [
    (100, {}, (50, 0.5, 35)),                     # int(100 * 0.5) = 50; ceil(log(0.01) / log(1 - 0.125)) = ceil(34.49) = 35
    (16, {}, (10, 0.625, 17)),                    # int(8.0) = 8 -> 10; epsilon 10/16; ceil(log(0.01) / log(1 - 0.244140625)) = ceil(16.45) = 17
    (10, {}, (10, 1.0, 1)),                       # min_inliers == N: one iteration
    (100, dict(max_iterations=20), (50, 0.5, 20)),
])
def test_plan_known_answers(N, over, want):
    got = R.plan(N, **dict(R.DEFAULT, **over))
    assert (got[0], float(got[1]), got[2]) == want


def test_plan_of_the_library_is_the_reference_plan():
    import ctypes as C
    from hyslam_amd import _native as N_
    lib = N_.lib()
    for N, eps, mi, mx, ms, pr in itertools.product((0, 4, 9, 10, 11, 16, 37, 100, 1000), (0.1, 0.4, 0.5, 0.9, 1.0), (4, 8, 10), (1, 20, 300), (4, 6), (0.5, 0.99)):
        par = N_.PnpParams(pr, mi, mx, ms, eps, 5.991, 1, 1, 0, 0, 0, 0)
        plan = N_.PnpPlan()
        assert lib.hs_pnp_plan(N, C.byref(par), C.byref(plan)) == N_.HS_OK
        want = R.plan(N, probability=pr, min_inliers=mi, max_iterations=mx, min_set=ms, epsilon=eps)
        got = (plan.min_inliers, np.float32(plan.epsilon), plan.max_iterations)
        assert got[0] == want[0] and got[2] == want[2] and (got[1] == want[1] or (np.isnan(got[1]) and np.isnan(want[1])) or N == 0), (N, eps, mi, mx, ms, pr, got, want)
    par = N_.PnpParams(0.99, 10, 300, 3, 0.5, 5.991, 1, 1, 0, 0, 0, 0)
    assert lib.hs_pnp_plan(100, C.byref(par), C.byref(N_.PnpPlan())) == N_.HS_ERR_INVALID, "min_set < 4"
    assert lib.hs_pnp_plan(100, None, None) == N_.HS_ERR_INVALID and lib.hs_pnp_plan(-1, C.byref(par), C.byref(N_.PnpPlan())) == N_.HS_ERR_INVALID


# ---------------------------------------------------------------- the sampler
def test_sampler_swaps_the_back_element_in():
    top = 0xFFFFFFFF
    assert R.sample(10, 4, [top, top, top, top]) == [9, 8, 7, 6]                 # the last index, each time of a shorter list
    assert R.sample(10, 4, [0, 0, 0, 0]) == [0, 9, 8, 7]                         # place 0 again: it holds the former back element
    assert R.sample(5, 4, [0, top, 0, top]) == [0, 3, 4, 1]                      # avail 01234 -> 4123 -> 412 -> 21 -> 2
    half = 1 << 31
    assert R.sample(8, 4, [half, half, half, half]) == [4, 3, 6, 2]              # places 4, 3, 3, 2 of 0123 4567 -> 0123 765 -> 012 675 -> 012 57
    for N, rows in ((16, [[0, 3, 6, 9], [15, 14, 0, 1]]), (40, [[39, 0, 1, 2]])):
        tab = PC.words_for(N, rows)
        for r, want in enumerate(rows):
            assert R.sample(N, 4, tab[r]) == want
    # the generator: element seed + it * min_set + k of hyslam_amd.synth.splitmix64(0, .), high word
    from hyslam_amd.synth import splitmix64
    z = splitmix64(0, 64)
    assert [R.draw32(5, 3, k, 4) for k in range(4)] == [int(z[5 + 12 + k] >> np.uint64(32)) for k in range(4)]
    assert R.draw32(5, 1, 2, 4, np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.uint32)) == 7 and R.draw32(5, 2, 0, 4, np.zeros((2, 4), np.uint32)) == R.draw32(5, 2, 0, 4)


# ---------------------------------------------------------------- the closed form of the loop against the loop as written, exhaustively
def _abstract(fn, counts, table, start, n, max_its, min_inliers=2):
    """one call over abstract hypotheses: hypothesis j has counts[j] inliers and is its own identity; table[id] says whether Refine() of that best
    set succeeds ('start' = the best set the state brings along)"""
    state = dict(start)
    it0 = state["iterations"]
    hyp = lambda it: (counts[it - it0], it - it0)
    refine = lambda best: (table[best], best)
    out = fn(state, n, 99, min_inliers, max_its, hyp, refine)
    distinct = []
    for b in out["refine_calls"]:
        if b not in distinct:
            distinct.append(b)
    return out["status"], out["at_iteration"], out["payload"], distinct, state["iterations"], state["best_inliers"], state["best"]


def test_records_form_equals_the_loop_exhaustively():
    checked = 0
    starts = [("none", dict(iterations=0, best_inliers=0, best=None), None),
              ("failed", dict(iterations=4, best_inliers=2, best="start"), False),
              ("refined", dict(iterations=4, best_inliers=2, best="start"), True),
              ("failed, exhausted", dict(iterations=9, best_inliers=3, best="start"), False)]
    for max_its in (1, 3, 6):
        for n in (1, 5, max_its + 2):
            for tag, start, start_ok in starts:
                passes = R.passes_of(start["iterations"], max_its, n)
                if passes > 6:
                    continue
                for counts in itertools.product(range(4), repeat=passes):
                    records = [j for j in range(passes) if counts[j] >= 2 and counts[j] > max([start["best_inliers"]] + list(counts[:j]))]
                    for outcome in itertools.product((False, True), repeat=len(records)):
                        table = dict(zip(records, outcome))
                        table["start"] = start_ok
                        a = _abstract(R.ransac_literal, counts, table, start, n, max_its)
                        b = _abstract(R.ransac_records, counts, table, start, n, max_its)
                        assert a == b, (tag, max_its, n, counts, table, a, b)
                        checked += 1
    assert checked > 20000
    # too few correspondences: nothing runs, in either form
    for fn in (R.ransac_literal, R.ransac_records):
        st = dict(iterations=0, best_inliers=0, best=None)
        assert fn(st, 5, 3, 4, 10, None, None)["status"] == R.TOO_FEW and st["iterations"] == 0


def test_the_loop_condition_is_an_or():
    for it0, max_its, n, want in ((0, 3, 5, 5), (0, 12, 5, 12), (4, 12, 5, 8), (12, 12, 5, 5), (20, 12, 1, 1)):
        assert R.passes_of(it0, max_its, n) == want
        st = dict(iterations=it0, best_inliers=0, best=None)
        R.ransac_literal(st, n, 99, 2, max_its, lambda it: (0, it), None)
        assert st["iterations"] == it0 + want


# ---------------------------------------------------------------- the decomposition and the poses
def test_jacobi_svd_against_numpy():
    rng = np.random.default_rng(5)
    for m, n in ((3, 3), (6, 3), (6, 4), (6, 5), (12, 12)):
        A = rng.normal(size=(m, n))
        if m == n == 12:
            B = rng.normal(size=(8, 12))
            A = B.T @ B                                            # rank 8: a null space of dimension four, as MtM of a minimal set has
        G, V, sig, perm = R.jacobi_svd(A)
        s = np.linalg.svd(A, compute_uv=False)
        assert np.allclose(sig[perm], s, rtol=1e-12, atol=1e-12 * s[0]) and list(sig[perm]) == sorted(sig, reverse=True)
        assert np.abs(V.T @ V - np.eye(n)).max() < 1e-13 and np.abs(G - A @ V).max() < 1e-12 * s[0]
        if m == n == 12:
            assert np.abs(A @ V[:, perm[8:]]).max() < 1e-12 * s[0], "the last four right singular vectors span the null space"
    assert np.allclose(R.pinv3(np.diag([2.0, 4.0, 8.0])), np.diag([0.5, 0.25, 0.125]))
    assert np.allclose(R.pinv_solve(np.eye(6)[:, :4], np.arange(6.0)), np.arange(4.0))


@pytest.mark.parametrize("name", NAMES)
def test_case_qualifies_and_literal_agrees_with_independent(name):
    """The qualification of the case, ASSERTED, and LITERAL against INDEPENDENT on it."""
    q = PC.qualify(name)
    print("%s: margins %s, spread under %d summation orders %.3g" % (name, {k: float("%.3g" % v) for k, v in q["margins"].items()}, PC.ORDERS, q["spread"]))
    for kind in PC.ASSERTED:                                       # error2, the sign of pcs[2], of det, and of b[0] in each of the three approximations
        assert q["margins"].get(kind, np.inf) >= PC.MARGIN, (kind, "decided within the margin", q["margins"].get(kind))
    assert set(q["margins"]) <= set(PC.ASSERTED) | set(PC.DEGENERATE), "a decision of a kind nobody classified"
    assert q["stable"], "flags, counts, status or at_iteration change with the summation order of the refine sums"
    assert q["spread"] <= PC.SPREAD_MEASURED, "the measured spread in tests/pnp_cases.py is out of date"
    # the decisions of PC.DEGENERATE (the `<` of the N = 1, 2, 3 choice; the b[1] and b[2] rules of approximations 2 and 3) cannot clear the margin on
    # consistent data, for the reason stated there; one decided within it is allowed only where it does not matter: both branches are then the same
    # pose to rounding, which is what the spread above measures with every such flip in it (see pnp_cases.IMMATERIAL)
    assert q["spread"] <= PC.IMMATERIAL
    lit = PC.expected(name)
    ind = PC.run(PC.cases()[name], kind="independent")
    assert PC.integer_outcome(lit) == PC.integer_outcome(ind), "flags, status or at_iteration differ between LITERAL and INDEPENDENT"
    for (a, _), (b, _) in zip(lit, ind):
        assert a["hypotheses_run"] == b["hypotheses_run"]
        if a["status"] == R.REFINED:                               # the refine poses only: a minimal-set hypothesis is basis-dependent by nature
            d = float(np.abs(a["Tcw_d"] - b["Tcw_d"]).max())
            print("%s: largest |LITERAL - INDEPENDENT| on the refine pose %.3g (tau %.3g)" % (name, d, PC.TAU))
            assert d <= PC.TAU
        carried = np.array_equal(a["Tcw_d"], a["Tcw"].astype(np.float64))      # a best from an earlier call: only its floats exist
        for T in (a["Tcw_d"],) if a["status"] in (R.REFINED, R.BEST) and not carried else ():
            Rm = T[:3, :3]
            assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rm) - 1.0) < 1e-12


def test_every_hypothesis_pose_is_a_rotation():
    """R R^T - I and det R - 1 below 1e-12 for every finite pose LITERAL forms on the cases: a product of two Jacobi-accumulated 3x3 rotations"""
    seen = 0
    for name in NAMES:
        s = PC.solver(PC.cases()[name])
        for it in range(min(s.max_its, 6)):
            if s.N < s.min_inliers:
                break
            Rm = s.hypothesis(it)[1][1]
            if np.all(np.isfinite(Rm)):
                assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rm) - 1.0) < 1e-12, (name, it)
                seen += 1
    assert seen > 30


def test_spread_constant_is_the_largest_measured():
    worst = max(PC.qualify(n)["spread"] for n in NAMES)
    print("largest deviation of LITERAL against itself under %d summation orders: %.3g; tau = 16 x = %.3g" % (PC.ORDERS, worst, 16 * worst))
    assert 0 < worst <= PC.SPREAD_MEASURED


def test_noise_free_hypotheses_against_the_data_itself():
    """A handle on the minimal-set EPnP that owes nothing to the transcription, on noise-free data.  EPnP on four points does NOT always find the pose:
    its four vectors span a null space whose basis is the decomposition's, and the three beta approximations assume the first of them dominates —
    with numpy.linalg's basis about half of the samples put their own four correspondences back within a pixel, the rest land anywhere (hundreds of
    pixels), and the reference's RANSAC lives with exactly that.  So what is asserted is (a) where a hypothesis does put its sample back within 1e-3 px,
    it is the camera: all 30 noise-free correspondences are inliers; (b) LITERAL succeeds (within a pixel) at least half as often as INDEPENDENT's EPnP
    on the same samples — a shared error in the kernel and its transcription would succeed never; (c) every scene has a success in 8 hypotheses."""
    fu, fv, uc, vc = [float(c) for c in PC.CAM]

    def worst(Rm, t, corrs, idx):
        X = corrs["Xw"][idx].astype(np.float64)
        with np.errstate(all="ignore"):
            Pc = np.stack([Rm[r, 0] * X[:, 0] + Rm[r, 1] * X[:, 1] + Rm[r, 2] * X[:, 2] + t[r] for r in range(3)], 1)
            e = np.hypot(corrs["u"][idx] - (uc + fu * Pc[:, 0] / Pc[:, 2]), corrs["v"][idx] - (vc + fv * Pc[:, 1] / Pc[:, 2])).max()
        return float(e) if np.isfinite(e) else np.inf

    lit, ind, exact = 0, 0, 0
    for seed in range(41, 47):
        corrs = PC.scene(seed, 30, 0.0, noise=0.0)[0]
        s = R.Solver(corrs, PC.CAM, dict(R.DEFAULT, max_iterations=8, seed=seed))
        here = 0
        for it in range(8):
            cnt, (_, Rm, t, _, idx) = s.hypothesis(it)
            e = worst(Rm, t, corrs, idx)
            here += e < 1.0
            ind += worst(*R.epnp_independent(R.points_of(corrs, idx), PC.CAM), corrs, idx) < 1.0
            if e < 1e-3:
                exact += 1
                assert cnt == 30, (seed, it, idx, e, cnt)
        assert here >= 1, (seed, "no hypothesis of 8 found the camera")
        lit += here
    print("noise-free minimal sets that reproject within a pixel: LITERAL %d, INDEPENDENT %d of 48; %d within 1e-3 px, each with all 30 inliers" % (lit, ind, exact))
    assert 2 * lit >= ind > 0 and exact >= 1
