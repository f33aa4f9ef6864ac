"""Directed and seeded cases for the batched EPnP RANSAC (tests/test_pnp_ref.py on the CPU, tests/test_gpu_pnp.py on the device).

A scene is landmarks in front of a known camera, seen with seeded sub-pixel pixel noise (it keeps the refine's small eigenvalues apart), some of
the matches replaced by gross outliers.  Everything is built from hyslam_amd.synth.splitmix64 with +, -, *, / and sqrt on float64 elementwise, so
the same bytes come out on every machine.

Every case records its QUALIFICATION (qualify): every error2 that any evaluated hypothesis or refine compares lies at least MARGIN (relative) from
its maxError, and flags, counts, status and at_iteration survive ORDERS seeded summation orders of the refine sums.  tests/test_pnp_ref.py ASSERTS it
for every case; it is never a filter.  The seeds below were chosen on the CPU so that it holds.

Asserted at MARGIN as well (ASSERTED below): the sign rule of solve_for_sign ("pc_sign": |pcs[2]| against |pc|, measured 0.81 .. 0.99), the sign of
det in estimate_R_and_t ("det_sign", measured 1.0) and the sign of b[0] in each of the three find_betas_approx ("beta_v1_b0", "beta_v2_b0",
"beta_v3_b0": |b[0]| against the largest |b|, measured 0.0075 .. 1).

Recorded under a key of their own but NOT required to clear MARGIN (DEGENERATE below), because on consistent data they cannot:
  - "choice", the two `<` of the N = 1, 2, 3 choice: the three approximations converge, under Gauss-Newton, to the same betas, so their reprojection
    errors agree to rounding (measured: decided by 1e-14 .. 2e-4 relative, 1e-14 .. 5e-13 on every case with a refine);
  - "beta_v2_b1", "beta_v2_b2", "beta_v3_b1", "beta_v3_b2", the rules on b[1] and b[2] of approximations 2 and 3: b[1] estimates beta1 * beta2 and b[2]
    beta2 squared, and where the vector of the smallest eigenvalue alone carries the solution (every refine over consistent inliers: EPnP's N = 1
    case) beta2 is zero to rounding (measured: 7e-7 .. 1e-5 of the largest |b| at the smallest, 0.03 .. 0.14 on the cases where beta2 matters).
Such a decision flips with the summation order and does not matter: both branches give the same pose to rounding.  What is asserted in their place is
exactly that: the largest deviation of a pose under the ORDERS orders, every such flip included, stays below IMMATERIAL, where a flip that mattered
(another local minimum, another sign of the camera) would show as a deviation of the size of the pose itself.

Measured (LITERAL against itself under the ORDERS summation orders, over all cases; tests/test_pnp_ref.py prints it): the largest deviation of a
Tcw_d entry is 1.155e-14, SPREAD_MEASURED below.  The device sums in point order, which is LITERAL's own order, and every operation on both sides
is a correctly rounded IEEE double operation, so the expected deviation of the device from LITERAL is zero: tests/test_gpu_pnp.py tests Tcw_d for
EQUALITY, and the device's largest deviation over the suite is 0.  TAU = 16 x SPREAD_MEASURED (the pose optimiser's protocol) is what LITERAL
against INDEPENDENT is held to on the refine poses (measured there: at most 2.4e-14).
"""
import functools

import numpy as np

import ref_pnp as R
from hyslam_amd.synth import splitmix64

MARGIN = 1e-4                    # the pose optimiser's margin (tests/poseopt_cases.py)
ORDERS = 8
ASSERTED = ("error2", "pc_sign", "det_sign", "beta_v1_b0", "beta_v2_b0", "beta_v3_b0")
DEGENERATE = ("choice", "beta_v2_b1", "beta_v2_b2", "beta_v3_b1", "beta_v3_b2")          # see the module docstring
SPREAD_MEASURED = 1.2e-14        # see the module docstring (1.155e-14 rounded up)
TAU = 16 * SPREAD_MEASURED
IMMATERIAL = 1e-9                # far above accumulated rounding (1e-14), far below any pose entry that a flipped decision which matters would move
CAM = (np.float32(520.0), np.float32(515.0), np.float32(320.5), np.float32(240.25))


def uniform(seed, n, stream):
    """n float64 in [0, 1) from the counter-based generator of hyslam_amd.synth"""
    return (splitmix64(seed, n, stream) >> np.uint64(11)).astype(np.float64) / float(1 << 53)


def rotation(seed):
    """a rotation of a few tenths of a radian from a seeded unit quaternion: sqrt and division only"""
    q = np.concatenate([[1.0], (uniform(seed, 3, 90) - 0.5) * 0.5])
    w, x, y, z = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scene(seed, N, outliers=0.25, noise=0.1, first_inliers=0):
    """(corrs CORR_DTYPE [N], Rcw, tcw).  outliers: a fraction (seeded choice) or an explicit index list; the first `first_inliers` correspondences
    are never outliers (directed draws aim at them)."""
    Rm = rotation(seed)
    t = (uniform(seed, 3, 91) - 0.5)
    Pc = np.stack([(uniform(seed, N, 92) - 0.5) * 4.0, (uniform(seed, N, 93) - 0.5) * 3.0, 3.0 + uniform(seed, N, 94) * 6.0], 1)
    d = Pc - t                                                     # Xw = R^T (Xc - t), written out: no BLAS summation order
    Xw = np.stack([Rm[0, j] * d[:, 0] + Rm[1, j] * d[:, 1] + Rm[2, j] * d[:, 2] for j in range(3)], 1)
    u = float(CAM[2]) + float(CAM[0]) * Pc[:, 0] / Pc[:, 2] + (uniform(seed, N, 95) - 0.5) * 2.0 * noise
    v = float(CAM[3]) + float(CAM[1]) * Pc[:, 1] / Pc[:, 2] + (uniform(seed, N, 96) - 0.5) * 2.0 * noise
    if isinstance(outliers, float):
        out = uniform(seed, N, 97) < outliers
        out[:first_inliers] = False
    else:
        out = np.zeros(N, bool)
        out[list(outliers)] = True
    u = np.where(out, uniform(seed, N, 98) * 640.0, u)
    v = np.where(out, uniform(seed, N, 99) * 480.0, v)
    c = np.zeros(N, R.CORR_DTYPE)
    c["Xw"], c["u"], c["v"], c["kp"] = Xw, u, v, np.arange(N) * 2 + 1
    level = (splitmix64(seed, N, 100) % np.uint64(8)).astype(np.int64)
    c["sigma2"] = (np.float32(1.2) ** level.astype(np.float32)) ** 2
    return c, Rm, t


def words_for(N, rows):
    """a draws table [len(rows), MAX_SET] of uint32 whose reduction (word * avail) >> 32 takes exactly the correspondences of each row, in order"""
    tab = np.zeros((len(rows), R.MAX_SET), np.uint32)
    for r, idxs in enumerate(rows):
        avail = list(range(N))
        for k, want in enumerate(idxs):
            pos = avail.index(want)
            w = -((-pos << 32) // len(avail))                      # the smallest word that reduces to pos
            assert (w * len(avail)) >> 32 == pos and w < (1 << 32)
            tab[r, k] = w
            avail[pos] = avail[-1]
            avail.pop()
    return tab


def _case(name, corrs, params, calls, draws=None):
    p = dict(R.DEFAULT, max_iterations=12, seed=0)
    p.update(params)
    return dict(name=name, corrs=corrs, cam=CAM, params=p, calls=list(calls), draws=draws)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # parity sizes: below the minimum, one iteration, a few, a wave, one past a wave, several per lane
    out.append(_case("n9_too_few", scene(11, 9, 0.0)[0], dict(seed=3), [5]))
    out.append(_case("n10_one_iteration", scene(12, 10, 0.0, noise=0.02)[0], dict(seed=1), [1]))
    out.append(_case("n12", scene(13, 12, [3, 8], noise=0.05)[0], dict(seed=4, epsilon=0.5), [12]))
    out.append(_case("n64", scene(14, 64, 0.25)[0], dict(seed=5), [12]))
    out.append(_case("n65", scene(15, 65, 0.25)[0], dict(seed=6), [12]))
    out.append(_case("n300", scene(16, 300, 0.3)[0], dict(seed=8), [12]))
    # past the 1024 correspondences whose compacted inliers k_pnp_select keeps in LDS: the refine's points go through the caller's work area.  The
    # table aims three hypotheses at inliers; the first misses min_inliers, the second refines (over 792 points)
    out.append(_case("n1100_work_area", scene(23, 1100, 0.3, noise=0.05, first_inliers=12)[0], dict(seed=15, max_iterations=4), [4],
                     words_for(1100, [[0, 3, 6, 9], [1, 4, 7, 10], [2, 5, 8, 11]])))
    # the loop's OR (:188): 3 planned and n = 5 runs 5; 12 planned and n = 5 runs 12.  All outliers: nothing returns early, the status is NONE
    junk = scene(17, 40, 1.0)[0]
    out.append(_case("or_max3_n5", junk, dict(seed=8, max_iterations=3), [5]))
    out.append(_case("or_max12_n5", junk, dict(seed=8, max_iterations=12), [5]))
    # the second call: after REFINED (the same pose at the first qualifying hypothesis), and on an exhausted problem
    out.append(_case("again_after_refined", scene(18, 48, 0.25)[0], dict(seed=9), [12, 12]))
    out.append(_case("again_exhausted", junk, dict(seed=10, max_iterations=4), [4, 3]))
    # BEST with a pose: 10 inliers of 16, min_inliers 10, so every refine lands exactly on min_inliers and fails its strict `>`; the draws table
    # aims iterations 0 and 2 at inliers, the generator serves the rest (draw_cap = 3 < 12).  Its second call is the one "after a failed refine".
    c16 = scene(19, 16, [10, 11, 12, 13, 14, 15], noise=0.02)[0]
    out.append(_case("best_refine_lands_on_min", c16, dict(seed=11), [12, 2], words_for(16, [[0, 3, 6, 9], [12, 1, 13, 2], [7, 2, 5, 8]])))
    # after a failed refine: three planned iterations, the second call's first hypothesis (iteration 3, still from the table) qualifies again
    out.append(_case("again_after_failed_refine", c16, dict(seed=14, max_iterations=3), [3, 2],
                     words_for(16, [[0, 3, 6, 9], [12, 1, 13, 2], [7, 2, 5, 8], [1, 4, 6, 8]])))
    # directed draws: the last index first, then repeated words (which, without replacement, take different correspondences)
    c40 = scene(20, 40, 0.2, first_inliers=8)[0]
    tab = words_for(40, [[39, 0, 1, 2], [4, 5, 6, 7]])
    tab = np.concatenate([tab, np.full((1, R.MAX_SET), 0xFFFFFFFF, np.uint32), np.zeros((1, R.MAX_SET), np.uint32)])
    out.append(_case("directed_draws", c40, dict(seed=12), [12], tab))
    # a non-finite correspondence: the status is one of the five and every loop ends
    bad = scene(21, 32, 0.2)[0].copy()
    bad["Xw"][5] = (np.nan, 1.0, 2.0)
    bad["u"][9] = np.inf
    out.append(_case("nonfinite_corr", bad, dict(seed=13), [12]))
    return {c["name"]: c for c in out}


BATCH = ("n12", "n9_too_few", "n65")     # three different N in one call, one of them TOO_FEW
# more problems than one launch pair takes (HS_PNP_BATCH = 16): the seventeenth goes to a second pair that shares the work area.  Every name here is
# called once with n = 12 and plans at most 12 iterations
BATCH17 = ("n12", "n64", "n65", "n300", "directed_draws", "nonfinite_corr", "again_after_refined", "best_refine_lands_on_min", "n9_too_few") * 2
BATCH17 = BATCH17[:17]


def solver(case, **kw):
    return R.Solver(case["corrs"], case["cam"], case["params"], case["draws"], **kw)


def run(case, **kw):
    """every call of the case: [(result of iterate, state snapshot after it)]"""
    s = solver(case, **kw)
    out = []
    for n in case["calls"]:
        r = s.iterate(n)
        out.append((r, dict(iterations=s.state["iterations"], best_inliers=s.state["best_inliers"], best_Tcw=s.best_Tcw.copy(), best_mask=s.best_mask.copy())))
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """LITERAL in point order: what the device is compared with.  Computed once and shared; the tests leave it unchanged."""
    return run(cases()[name])


def integer_outcome(calls):
    return [(r["status"], r["n_inliers"], r["at_iteration"], r["iterations"], r["refines_run"], None if r["mask"] is None else r["mask"].tobytes(),
             st["best_inliers"], st["best_mask"].tobytes()) for r, st in calls]


@functools.lru_cache(maxsize=None)
def qualify(name):
    """dict(margins: {kind: smallest relative margin}, stable: integer outcome equal under ORDERS orders, spread: largest |Tcw_d| deviation)"""
    case = cases()[name]
    mg = R.Margins()
    base = run(case, margins=mg)
    stable, spread = True, 0.0
    for o in range(ORDERS):
        other = run(case, order_seed=1000 + o)
        stable = stable and integer_outcome(other) == integer_outcome(base)
        for (a, _), (b, _) in zip(base, other):
            if a["status"] in (R.REFINED, R.BEST) and b["status"] == a["status"]:
                spread = max(spread, float(np.abs(a["Tcw_d"] - b["Tcw_d"]).max()))
    return dict(margins=dict(mg.m), stable=stable, spread=spread)
