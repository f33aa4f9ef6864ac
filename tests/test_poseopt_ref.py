"""CPU: pins tests/ref_poseopt.py (Optimizer::PoseOptimization restated) independently of the library, and the cases of tests/poseopt_cases.py.

  - the literal and the array version agree bit for bit, in g2o's order and under a permuted summation order
  - the analytic Jacobians agree with central differences of the restated error function under exp(dx) * T
  - a problem whose residuals are exactly zero keeps every inlier and returns the quaternion round trip of its input pose, bit for bit
  - round 3 (no kernel, fixed inlier set) ends where scipy's Levenberg-Marquardt ends, within a bound made of both solvers' final gradients
  - every case qualifies, the directed cases take the paths they are named after, and tests/golden/poseopt_cases.npz is what the generators give
"""
import math

import numpy as np
import pytest

import poseopt_cases as P
import ref_poseopt as R

COUNTERS = ("n_edges", "n_good", "rounds", "lm_iterations", "lm_trials", "status", "max_trials", "empty_rounds")


def same(a, b):
    assert all(a[k] == b[k] for k in COUNTERS), [(k, a[k], b[k]) for k in COUNTERS]
    assert np.array_equal(a["round_flags"], b["round_flags"]) and np.array_equal(a["outlier"], b["outlier"])
    assert a["Tcw_d"].tobytes() == b["Tcw_d"].tobytes() and a["Tcw"].tobytes() == b["Tcw"].tobytes()
    assert a["min_margin"] == b["min_margin"]


@pytest.mark.parametrize("name", ["n3", "n9", "n10", "n65", "n257", "mono_out30", "stereo_out15", "mixed_out15", "all_outliers_round", "inlier_again",
                                  "ten_rejections"])
def test_literal_equals_fast(name):
    c = P.case(name)
    same(R.pose_optimization_literal(c["T"], c["cam"], c["edges"]), c["ref"])
    perm = P.perms(len(c["edges"]))[3]
    same(R.pose_optimization_literal(c["T"], c["cam"], c["edges"], perm), R.pose_optimization_fast(c["T"], c["cam"], c["edges"], perm))


def test_fast_and_literal_evaluators_agree_on_the_system():
    c = P.case("mixed_out15")
    T = R.se3_from_pose(c["T"])
    order = [int(i) for i in P.perms(len(c["edges"]))[0][:77]]
    for robust in (True, False):
        a, b = R._Literal(c["cam"], c["edges"]).system(T, order, robust), R._Fast(c["cam"], c["edges"]).system(T, order, robust)
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
        assert R._Literal(c["cam"], c["edges"]).robust_chi(T, order, robust) == R._Fast(c["cam"], c["edges"]).robust_chi(T, order, robust)


@pytest.mark.parametrize("stereo", [False, True])
def test_jacobians_against_central_differences(stereo):
    """J = d error / d dx at dx = 0 for estimate = exp(dx) * T.  The mono error is all double: step 1e-5, and the bound is the truncation term
    h^2 |J| (the derivatives of a projection grow like J itself for these depths) plus the rounding of a ~1e3 px value, 1e3 * 2^-52 / h.  The stereo
    error goes through a float invz, which moves a projected coordinate by up to 2^-24 of its value (<= 1280 px): the rounding term becomes
    1280 * 2^-24 / h, and h = 1e-2 balances it against the truncation term."""
    c = P.case("mixed_out0")
    T = R.se3_from_pose(c["T"])
    cam = [float(v) for v in c["cam"]]
    h = 1e-2 if stereo else 1e-5
    checked = 0
    for e in c["edges"][:40]:
        if (not e["ur"] < 0) != stereo:
            continue
        X, obs = [float(v) for v in e["Xw"]], [float(e["u"]), float(e["v"]), float(e["ur"])]
        J = np.array(R.edge_jacobian(T, X, cam, stereo))
        num = np.zeros_like(J)
        for j in range(6):
            d = [0.0] * 6
            d[j] = h
            ep = np.array(R.edge_error(R.se3_exp(d).mul(T), X, obs, cam, stereo))
            d[j] = -h
            em = np.array(R.edge_error(R.se3_exp(d).mul(T), X, obs, cam, stereo))
            num[:, j] = (ep - em) / (2 * h)
        scale = np.abs(J).max()
        bound = h * h * scale + (1280.0 * 2.0 ** -24 if stereo else 1e3 * 2.0 ** -52) / h
        assert np.abs(num - J).max() <= bound, (np.abs(num - J).max(), bound)
        assert bound < 2e-4 * scale                               # the bound itself is tight enough to catch a wrong sign or a swapped entry
        checked += 1
    assert checked >= 10


def _exact_problem():
    """identity pose, depths that are powers of two, coordinates with few bits: every projection is exact in float, every residual exactly zero"""
    fx, fy, cx, cy, bf = P.CAM
    rng = np.random.default_rng(5)
    n = 24
    z = 2.0 ** rng.integers(1, 5, n)
    x, y = rng.integers(-12, 13, n) * 0.125, rng.integers(-8, 9, n) * 0.125
    e = np.zeros(n, R.EDGE_DTYPE)
    e["Xw"] = np.stack([x, y, z], 1)
    e["u"], e["v"] = x / z * fx + cx, y / z * fy + cy
    e["ur"] = np.where(np.arange(n) % 3 == 0, -1.0, x / z * fx + cx - bf / z)
    e["inv_sigma2"], e["kp"] = 1.0, np.arange(n)
    assert np.array_equal(e["u"].astype(np.float64), x / z * fx + cx) and (e["ur"][np.arange(n) % 3 != 0] >= 0).all()
    return np.eye(4, dtype=np.float32), np.array(P.CAM, np.float32), e


def test_zero_residuals_leave_the_round_trip_of_the_input():
    T, cam, e = _exact_problem()
    for fn in (R.pose_optimization_literal, R.pose_optimization_fast):
        r = fn(T, cam, e)
        assert r["n_good"] == len(e) and not r["outlier"].any() and r["rounds"] == 4
        # chi = 0: dx = 0, rho = 0 / 1e-3 = 0 — the step is rejected and the iteration terminates: one iteration of one trial per round
        assert (r["lm_iterations"], r["lm_trials"]) == (4, 4)
        assert r["Tcw_d"].tobytes() == R.se3_from_pose(T).matrix().tobytes() == np.eye(4).tobytes()


def test_noiseless_start_at_the_truth_keeps_every_inlier():
    """a general pose: the observations are rounded to float (<= 1280 * 2^-24 px = 7.6e-5 px), so the optimum moves from the input by about that over
    fx in angle and that times the largest depth (25) over fx in translation: 2.7e-6; the pose stays within ten times that of the round trip"""
    c = P.case("ten_rejections")
    r = c["ref"]
    assert r["n_good"] == len(c["edges"]) and not r["round_flags"].any()
    assert np.abs(r["Tcw_d"] - R.se3_from_pose(c["T"]).matrix()).max() <= 10 * 25 * 1280 * 2.0 ** -24 / 700


def _local_delta(Ta, Tb):
    """dx with Ta ~= exp(dx) * Tb, to first order"""
    M = Ta @ np.linalg.inv(Tb) - np.eye(4)
    return np.array([(M[2, 1] - M[1, 2]) / 2, (M[0, 2] - M[2, 0]) / 2, (M[1, 0] - M[0, 1]) / 2, M[0, 3], M[1, 3], M[2, 3]])


@pytest.mark.parametrize("name", ["mono_out15", "mixed_out15"])
def test_round_three_against_scipy_lm(name):
    """Round 3 minimises sum chi2 over the inliers of round 2 from the input pose, without a kernel.  scipy's MINPACK Levenberg-Marquardt minimises the
    same residuals sqrt(w) e over x with estimate = exp(x) * input.  Two points with gradients g1, g2 of a function whose Hessian is at least
    lambda_min lie within (|g1| + |g2|) / lambda_min of each other; H = J^T J is the Hessian but for the residual-curvature term, for which the bound
    is doubled."""
    from scipy.optimize import least_squares
    c = P.case(name)
    ref = c["ref"]
    assert ref["rounds"] == 4
    idx = [int(i) for i in np.nonzero(ref["round_flags"][2] == 0)[0]]
    cam, e = [float(v) for v in c["cam"]], c["edges"]
    T0 = R.se3_from_pose(c["T"])
    X = [[float(v) for v in e["Xw"][i]] for i in idx]
    obs = [[float(e["u"][i]), float(e["v"][i]), float(e["ur"][i])] for i in idx]
    st = [not (e["ur"][i] < 0) for i in idx]
    sw = [math.sqrt(float(e["inv_sigma2"][i])) for i in idx]

    def residuals(T):
        return np.array([sw[k] * v for k in range(len(idx)) for v in R.edge_error(T, X[k], obs[k], cam, st[k])])

    def jacobian(T):
        return np.array([[sw[k] * v for v in row] for k in range(len(idx)) for row in R.edge_jacobian(T, X[k], cam, st[k])])

    # edge_jacobian is the derivative at x = 0 only, and the stereo error's float invz makes numerical differences useless: scipy gets the local
    # Jacobian and is re-centred (x = 0 at its last answer) until its answer stays put, so that the Jacobian is exact where it ends
    T_sp = T0
    for _ in range(5):
        base = T_sp
        sol = least_squares(lambda x: residuals(R.se3_exp(list(x)).mul(base)), np.zeros(6), jac=lambda x: jacobian(R.se3_exp(list(x)).mul(base)),
                            method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
        T_sp = R.se3_exp(list(sol.x)).mul(base)
    T_ref = R.SE3(R.Quat.from_matrix(ref["Tcw_d"][:3, :3].tolist()), ref["Tcw_d"][:3, 3].tolist())
    J = jacobian(T_ref)
    g_ref, g_sp = J.T @ residuals(T_ref), jacobian(T_sp).T @ residuals(T_sp)
    lam_min = float(np.linalg.eigvalsh(J.T @ J)[0])
    bound = 2 * (np.linalg.norm(g_ref) + np.linalg.norm(g_sp)) / lam_min
    delta = np.linalg.norm(_local_delta(T_sp.matrix(), ref["Tcw_d"]))
    print("%s: |delta| %.3e, bound %.3e (|g_ref| %.3e, |g_scipy| %.3e, lambda_min %.3e)" % (name, delta, bound, np.linalg.norm(g_ref), np.linalg.norm(g_sp), lam_min))
    assert delta <= bound
    # the bound says something: it is below a hundredth of the distance the round covered, so a solver that stopped on the way fails.  (With stereo
    # edges the float invz leaves gradients of ~0.1 .. 5 at both answers — the objective has steps of 1e-4 px — and the bound is that much looser.)
    assert bound < 1e-2 * np.linalg.norm(_local_delta(T0.matrix(), ref["Tcw_d"]))


def test_every_case_qualifies_and_the_tolerance_is_small_enough():
    spread = 0.0
    for name in sorted(P.SPECS):
        c = P.case(name)                                          # raises when no seed qualifies
        assert c["ref"]["min_margin"] >= P.MARGIN and c["ref"]["n_edges"] == P.SPECS[name][0]
        spread = max(spread, c["spread"])
    tau = P.TAU_FACTOR * spread
    print("largest deviation of the reference from itself under %d summation orders: %.3e; tau = %d x = %.3e" % (P.N_PERM, spread, P.TAU_FACTOR, tau))
    assert 0 < tau < 3e-9                                         # a tenth of half a float32 ulp at 1.0; above it the case set is wrong, not the bound


def test_directed_cases_take_their_paths():
    for n in P.TOO_FEW:                                           # nInitialCorrespondences < 3
        T, cam, e = P.too_few(n)
        r = R.pose_optimization_literal(T, cam, e)
        assert (r["status"], r["n_good"], r["rounds"], r["n_edges"], r["outlier"]) == (R.STATUS_TOO_FEW, 0, 0, n, None)
        assert r["Tcw"].tobytes() == T.tobytes() and np.array_equal(r["Tcw_d"], T.astype(np.float64))
    assert P.case("n3")["ref"]["rounds"] == 1 and P.case("n9")["ref"]["rounds"] == 1 and P.case("n10")["ref"]["rounds"] == 4     # edges().size() < 10
    r = P.case("all_outliers_round")["ref"]
    assert r["round_flags"][0].all() and r["empty_rounds"] == 3 and r["n_good"] == 0
    assert r["Tcw_d"].tobytes() == R.se3_from_pose(P.case("all_outliers_round")["T"]).matrix().tobytes()    # an empty round leaves the input pose
    r = P.case("inlier_again")["ref"]
    assert ((r["round_flags"][0] == 1) & (r["outlier"] == 0)).any()
    assert P.case("ten_rejections")["ref"]["max_trials"] == 10


def test_errors_belong_to_the_last_evaluated_estimate():
    """after a rejected trial the estimate is restored but the edges keep the errors of the rejected trial (D14): the optimiser hands back both
    states, and the classification reads the inliers' chi2 at the second.  After TEN rejections lambda has grown by 2^55, the rejected step is below
    the rounding of the pose, and the two states are numerically the same pose — which is why the rule costs the device nothing but a second
    variable; where an iteration ends on rho == 0 they may differ."""
    c = P.case("ten_rejections")
    ev = R._Fast([np.float32(v) for v in c["cam"]], c["edges"])
    st = dict(lm_iterations=0, lm_trials=0, max_trials=0)
    T, T_err = R._levenberg(ev, R.se3_from_pose(c["T"]), list(range(len(c["edges"]))), True, st)
    assert st["max_trials"] == 10 and T_err is not T
    assert np.abs(np.array(T_err.key()) - np.array(T.key())).max() <= 2.0 ** -50


def test_golden_file_is_what_the_generators_give():
    want, have = P.golden_arrays(), P.load_golden()
    assert sorted(want) == sorted(have)
    tau = float(have["tau"])
    assert tau == P.TAU_FACTOR * float(have["spread"]) and abs(float(want["spread"]) - float(have["spread"])) <= 0.1 * float(have["spread"]) and P.TAU_FACTOR * float(want["spread"]) < 3e-9
    for k in want:
        if k in ("spread", "tau"):
            continue
        a, b = np.asarray(want[k]), np.asarray(have[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if k.endswith(".Tcw_d"):
            assert np.abs(a - b).max() <= tau, k                  # another libm may move the last bits; never more than the reference moves itself
        elif k.endswith(".Tcw"):
            assert np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max() <= 1, k
        else:
            assert a.tobytes() == b.tobytes(), k
