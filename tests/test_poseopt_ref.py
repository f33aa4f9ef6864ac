"""CPU: pins tests/ref_poseopt.py (Optimizer::PoseOptimization restated) independently of the library, and the cases of tests/poseopt_cases.py.

  - the literal and the array version agree bit for bit, in g2o's order and under a permuted summation order
  - the analytic Jacobians agree with central differences of the restated error function under exp(dx) * T
  - a problem whose residuals are exactly zero keeps every inlier and returns the quaternion round trip of its input pose, bit for bit
  - round 3 (no kernel, fixed inlier set) ends where scipy's Levenberg-Marquardt ends, within a bound made of both solvers' final gradients
  - Quat.from_matrix off its trace branch takes the branch Eigen's rule names and agrees with scipy's quaternion, at and near 180 degrees
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
                                  "ten_rejections"] + list(P.ADDED))
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
    _jacobians_against_central_differences("mixed_out0", stereo)


@pytest.mark.parametrize("stereo", [False, True])
def test_jacobians_with_an_anisotropic_camera(stereo):
    """the same with fx = 700, fy = 520: a focal length taken from the other axis is off by a quarter of the entry, far above the bound"""
    _jacobians_against_central_differences("fxfy_stereo" if stereo else "fxfy_mono", stereo)


def _jacobians_against_central_differences(name, stereo):
    c = P.case(name)
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


def _quat_sweep():
    """rotations with trace <= 0: the exact half turns about the axes, the face diagonals and the space diagonal (their diagonal entries tie), and
    seeded rotations of 121 .. 180 degrees about random axes"""
    out = []
    for k in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)):
        k = np.array(k, np.float64) / math.sqrt(sum(k))
        out.append(2.0 * np.outer(k, k) - np.eye(3))
    rng = np.random.default_rng(77)
    for _ in range(600):
        k = rng.normal(0, 1, 3)
        out.append(P._rot(k / np.linalg.norm(k) * np.deg2rad(rng.uniform(121.0, 180.0))))
    return out


def test_quaternion_of_a_matrix_off_the_trace_branch():
    """Quat.from_matrix on the sweep: the branch is the one P.quat_branch (Eigen's rule: trace <= 0, then m11 > m00, then m22 > max) predicts — the
    component the branch sets directly is 0.5 sqrt(m_ii - m_jj - m_kk + 1) bit for bit —, the quaternion is scipy's up to sign, and matrix() gives
    the rotation back.  Measured over the sweep: 2.2e-16 against scipy, 1.0e-15 round trip; the bound is four times the larger, 4e-15.  A wrong sign or permutation misses by order 1."""
    from scipy.spatial.transform import Rotation
    taken, worst_q, worst_m = [0, 0, 0], 0.0, 0.0
    for m in _quat_sweep():
        assert np.trace(m) <= 0.0
        i = P.quat_branch(m.tolist())
        j, k = (i + 1) % 3, (i + 2) % 3
        q = R.Quat.from_matrix(m.tolist())
        v = [q.x, q.y, q.z]
        assert v[i] == 0.5 * math.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0) and m[i, i] >= m[j, j] and m[i, i] >= m[k, k]
        taken[i] += 1
        mine, theirs = np.array(v + [q.w]), Rotation.from_matrix(m).as_quat()
        worst_q = max(worst_q, min(np.abs(mine - theirs).max(), np.abs(mine + theirs).max()))
        worst_m = max(worst_m, np.abs(np.array(q.matrix()) - m).max())
    print("branches taken %s; worst against scipy %.3e, worst round trip %.3e" % (taken, worst_q, worst_m))
    assert min(taken) >= 100
    assert worst_q <= 4e-15 and worst_m <= 4e-15


def test_zero_residuals_leave_the_round_trip_of_the_input():
    T, cam, e = P.exact_problem()
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


@pytest.mark.parametrize("name", ["mono_out15", "mixed_out15", "fxfy_mono", "rot_i1"])
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
    # the start pose's rotation leaves Quat.from_matrix by the branch the case is named after; the camera of these cases has fx != fy
    for tag, lo, hi in (("rot", -1.0, -0.9), ("rot_125", -0.3, 0.0)):
        for i in range(3):
            c = P.case("%s_i%d" % (tag, i))
            m = c["T"].astype(np.float64)[:3, :3]
            assert lo <= np.trace(m) <= hi and P.quat_branch(m) == i and m[i, i] > max(m[j, j] for j in range(3) if j != i)
            assert tuple(c["cam"]) == tuple(np.float32(P.CAM_ANISO)) and c["ref"]["rounds"] == 4
    m = P.case("rot_tie")["T"].astype(np.float64)[:3, :3]
    assert np.trace(m) <= 0 and abs(m[0, 0] - m[1, 1]) <= 1e-3 and m[2, 2] < -0.99 and P.quat_branch(m) in (0, 1)
    for name in ("fxfy_mono", "fxfy_stereo", "behind_camera"):
        assert tuple(P.case(name)["cam"]) == tuple(np.float32(P.CAM_ANISO))
    # every factorisation fails (H = 0, lambda = 0, the first pivot 0 <= 0): the step is the last dx = 0, temp = DBL_MAX, ten rejections an iteration
    c = P.case("zero_information")
    r, n = c["ref"], len(c["edges"])
    assert n == 40 and not c["edges"]["inv_sigma2"].any()
    assert (r["rounds"], r["lm_iterations"], r["lm_trials"], r["n_good"], r["max_trials"]) == (4, 4, 40, n, 10) and not r["round_flags"].any()
    assert r["Tcw_d"].tobytes() == R.se3_from_pose(c["T"]).matrix().tobytes()
    c = P.case("some_zero_information")
    r, zero = c["ref"], c["aux"]["zero"]
    assert np.array_equal(np.nonzero(c["edges"]["inv_sigma2"] == 0)[0], zero) and len(zero) == 40
    assert not r["outlier"][zero].any() and len(np.intersect1d(zero, c["aux"]["bad"])) > 0 and r["outlier"].any()
    # zero residuals: chi = 0, dx = 0, rho = 0 / 1e-3 = 0 — rejected, and the iteration is the last (the other half of D14)
    c = P.case("exact_zero")
    r = c["ref"]
    assert c["edges"].tobytes() == P.exact_problem()[2].tobytes()
    assert (r["rounds"], r["lm_iterations"], r["lm_trials"], r["n_good"]) == (4, 4, 4, len(c["edges"])) and not r["round_flags"].any()
    # points behind the camera: no depth test, so a consistent observation is an inlier with invz < 0
    c = P.case("behind_camera")
    r, mirrored = c["ref"], c["aux"]
    z = c["edges"]["Xw"].astype(np.float64) @ r["Tcw_d"][2, :3] + r["Tcw_d"][2, 3]
    assert len(mirrored) == 24 and (z[mirrored] < 0).all() and (np.delete(z, mirrored) > 0).all()
    assert (r["outlier"][mirrored] == 0).any() and (r["outlier"][mirrored] == 1).any()
    print("behind_camera: %d of %d mirrored edges are inliers" % (int((r["outlier"][mirrored] == 0).sum()), len(mirrored)))
    # ur = +0.0f and -0.0f are stereo by !(ur < 0)
    c = P.case("ur_zero")
    ur = c["edges"]["ur"][c["aux"]]
    assert len(ur) == 2 * P.N_SIGNED_ZERO and (ur == 0).all() and int(np.signbit(ur).sum()) == P.N_SIGNED_ZERO
    lit = R._Literal(c["cam"], c["edges"])
    assert all(lit.stereo[i] for i in c["aux"]) and R._Fast(c["cam"], c["edges"]).stereo[c["aux"]].all()
    assert (c["ref"]["outlier"][c["aux"]] == 0).any()             # ... and fit as stereo edges: read as mono they would leave a pose that rejects none
    for name in P.DIRECTED:
        assert name in P.SPECS


def test_chain_problem_qualifies_and_is_what_the_gather_gives():
    """the 2049-keypoint frame of the GPU chain test: its edge list qualifies like a case (margin, flags under 8 orders, spread within SPREAD_CAP),
    and gathering from its arrays gives that list back"""
    c = P.chain_problem()
    q = P.qualify(c["T"], c["cam"], c["edges"], spread_cap=P.SPREAD_CAP)
    assert q is not None and q[0]["rounds"] == 4 and 0 < q[0]["n_good"] < P.CHAIN_N
    got, count = R.gather_edges(c["kps"], c["uR"], c["kp_lm"], c["lm_pos"])
    assert count == P.CHAIN_N and got.tobytes() == c["edges"].tobytes()
    assert (c["uR"] < 0).any() and (c["uR"] >= 0).any()


def test_reference_gather_equals_the_python_gather():
    """ref_poseopt.gather_edges against Optimizer.pose_edges on every synthetic frame the GPU test gives hs_pose_edges_device, with another size_ref
    and sigma_ref, a keypoint of infinite size (weight 0), no keypoint and no landmark.  Two statements of one loop: the same bytes."""
    from hyslam_amd.features import Optimizer
    frames = [P.edge_frame(n, v) for n in P.EDGE_FRAME_SIZES for v in P.EDGE_FRAME_VARIANTS]
    f = P.edge_frame(2049, "sparse")
    f["kps"]["size"][P.EDGE_CHUNK] = np.inf
    frames.append(f)
    frames.append({k: v[:0] if k != "lm_pos" else v for k, v in P.edge_frame(1023, "all").items()})     # F.n = 0
    frames.append(dict(P.edge_frame(1025, "all"), lm_pos=np.zeros((0, 3), np.float32)))                   # L = 0
    counts = []
    for f in frames:
        for size_ref, sigma_ref in ((31.0, 1.0), (24.5, 1.7)):
            want, count = R.gather_edges(f["kps"], f["uR"], f["kp_lm"], f["lm_pos"], size_ref=size_ref, sigma_ref=sigma_ref)
            got = Optimizer.pose_edges(f["kps"], f["uR"], f["kp_lm"], f["lm_pos"], size_ref=size_ref, sigma_ref=sigma_ref)
            assert count == len(want) == len(got) and want.tobytes() == got.tobytes()
            assert np.array_equal(want["kp"], np.nonzero((f["kp_lm"] >= 0) & (f["kp_lm"] < len(f["lm_pos"])))[0])
        counts.append(count)
    assert counts[-2:] == [0, 0] and 0 in counts[:-2] and 3000 in counts
    f = frames[-3]
    e, _ = R.gather_edges(f["kps"], f["uR"], f["kp_lm"], f["lm_pos"])
    assert e["inv_sigma2"][e["kp"] == P.EDGE_CHUNK].tobytes() == np.float32(0.0).tobytes()
    # sigma_ref * (s * s), not (sigma_ref * s) * s: with sigma_ref = 1.7 the two differ in the last bit on some size
    s = f["kps"]["size"][e["kp"]] / np.float32(24.5)
    a, b = np.float32(1.0) / (np.float32(1.7) * (s * s)), np.float32(1.0) / ((np.float32(1.7) * s) * s)
    assert (a[np.isfinite(s)] != b[np.isfinite(s)]).any()


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
