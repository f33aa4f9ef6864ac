"""Inputs of the pose-only optimisation tests (tests/test_poseopt_ref.py, tests/test_gpu_poseopt.py): seeded generators and directed cases.

A scene is a camera like the bench's (fx = fy = 700, 1280x720, bf = 84), points 2..25 units in front of a true pose, a start pose a few cm / ~0.5
degrees off, keypoint sizes 31 * 1.2^level, pixel noise scaled by the level and a chosen share of gross outliers.  Every input is rounded to
float32, as the C ABI carries it.  scene() also takes the true rotation (an axis-angle vector) and the camera; the special cases below are scenes
edited after the draw (weights set to zero, points mirrored behind the camera, ur = +-0) or the fixed problem of exact_problem().

A case QUALIFIES when, in the reference (ref_poseopt.pose_optimization_fast), every classification of every round has |chi2/th - 1| >= MARGIN and
the flags of all rounds are identical under N_PERM seeded summation orders.  A generator draws the next seed until its case qualifies and any
directed property holds (`want`), so what a name stands for is fixed by this file alone.  A case's first seed is fixed by name (FROZEN, ADDED): a
new name never moves an older case.  A name of ADDED qualifies only with a spread of at most SPREAD_CAP, so tau stays what the FROZEN names made
it.  tests/golden/poseopt_cases.npz holds the inputs and the reference's outputs of every case; the GPU tests read the cases from that file alone.
edge_frame() and chain_problem() are the synthetic frames of the edge-gather tests: a few arrays from a fixed seed, regenerated where they are used."""
import functools
import os

import numpy as np

import ref_poseopt as R

CAM = (700.0, 700.0, 640.0, 360.0, 84.0)
CAM_ANISO = (700.0, 520.0, 640.0, 360.0, 84.0)                  # fx != fy: a mixed-up focal length in the error or a Jacobian entry shows
WIDTH, HEIGHT = 1280, 720
MARGIN, N_PERM, TAU_FACTOR = 1e-4, 8, 16
SPREAD_CAP = 1.3e-10                                            # just below the largest spread of the FROZEN names (1.316e-10, which sets tau)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseopt_cases.npz")
BLOCK = 256                                                     # k_pose_optimize's workgroup (HS_POSE_THREADS)

# name -> (edge count, kind, outlier share, start offset scale, noise scale, directed property)
SPECS = {}
for _n in (3, 9, 10, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 1000):
    SPECS["n%d" % _n] = (_n, "mixed", 0.15, 1.0, 1.0, None)
for _kind in ("mono", "stereo", "mixed"):
    for _share in (0, 15, 30):
        SPECS["%s_out%d" % (_kind, _share)] = (120, _kind, _share / 100.0, 1.0, 1.0, None)
SPECS["all_outliers_round"] = (40, "mixed", 1.0, 1.0, 1.0, "empty_round")       # after round 0 every edge is an outlier: round 1 has no active edge
SPECS["inlier_again"] = (150, "mixed", 0.3, 4.0, 1.0, "inlier_again")           # an outlier of round 0 is an inlier at the end
SPECS["ten_rejections"] = (80, "mixed", 0.0, 0.0, 0.0, "ten_rejections")        # noiseless, started at the optimum: an iteration spends all 10 trials
SPECS["batch_257"] = (257, "mixed", 0.15, 1.0, 1.0, None)
SPECS["batch_12"] = (12, "stereo", 0.15, 1.0, 1.0, None)
BATCH = ("batch_257", None, "batch_12")                         # Q = 3 with sizes (257, 0, 12); None = a problem without edges
TOO_FEW = (0, 2)                                                # edge counts below 3: not optimised
# the names above in sorted order, as they stood when their seeds were first drawn: name i starts at seed 7919 * (i + 1).  Never edited.
FROZEN = ("all_outliers_round", "batch_12", "batch_257", "inlier_again", "mixed_out0", "mixed_out15", "mixed_out30", "mono_out0", "mono_out15",
          "mono_out30", "n10", "n1000", "n255", "n256", "n257", "n3", "n63", "n64", "n65", "n9", "stereo_out0", "stereo_out15", "stereo_out30",
          "ten_rejections")
assert sorted(SPECS) == list(FROZEN)

# ---- cases for the branches the scenes above never reach.  Eigen's Quaterniond(Matrix3d), which the start pose and every exp() go through, takes
# the trace branch for trace > 0 and otherwise the largest diagonal entry: i = 0; if m11 > m00: i = 1; if m22 > m[i][i]: i = 2  (quat_branch).
TILT = (0.03, -0.02, 0.05)
SCENE_ARGS = {}                                                 # name -> scene()'s rot / cam
for _deg, _tag in ((175, "rot"), (125, "rot_125")):
    for _i in range(3):
        _w = np.array(TILT)
        _w[_i] += np.deg2rad(_deg)                              # _deg about x, y, z and the tilt: the largest diagonal entry is m[_i][_i]
        SPECS["%s_i%d" % (_tag, _i)] = (120, "mixed", 0.15, 1.0, 1.0, "branch_i%d" % _i)
        SCENE_ARGS["%s_i%d" % (_tag, _i)] = dict(rot=tuple(_w), cam=CAM_ANISO)
SPECS["rot_tie"] = (120, "mixed", 0.15, 1.0, 1.0, "tie")       # 180 degrees about (1, 1, 0) / sqrt 2: m00 = m11 = 0 but for the tilt and the start offset
SCENE_ARGS["rot_tie"] = dict(rot=tuple(np.pi * np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0) + np.array([2e-4, -1e-4, 1e-4])), cam=CAM)
SPECS["fxfy_mono"] = (120, "mono", 0.15, 1.0, 1.0, None)
SPECS["fxfy_stereo"] = (120, "stereo", 0.15, 1.0, 1.0, None)
SCENE_ARGS["fxfy_mono"] = SCENE_ARGS["fxfy_stereo"] = dict(cam=CAM_ANISO)
SPECS["zero_information"] = (40, "mixed", 0.15, 1.0, 1.0, "zero_information")             # inv_sigma2 = 0 on every edge: H = 0, every factorisation fails
SPECS["some_zero_information"] = (120, "mixed", 0.15, 1.0, 1.0, "some_zero_information")  # inv_sigma2 = 0 on every third edge
SPECS["exact_zero"] = (24, "mixed", 0.0, 0.0, 0.0, "exact_zero")                          # exact_problem(): every iteration ends on rho == 0
SPECS["behind_camera"] = (120, "mixed", 0.15, 1.0, 1.0, "behind_camera")                  # a fifth of the points behind the camera, observed consistently
SCENE_ARGS["behind_camera"] = dict(cam=CAM_ANISO)
SPECS["ur_zero"] = (120, "mixed", 0.15, 1.0, 1.0, "ur_zero")                              # stereo edges whose ur is +0.0f and -0.0f
# first seeds of the names added after FROZEN, in the order they were added (append only): name k starts at 1000003 * (k + 1), far above 7919 * 24 + 400
ADDED = ("rot_i0", "rot_i1", "rot_i2", "rot_125_i0", "rot_125_i1", "rot_125_i2", "rot_tie", "fxfy_mono", "fxfy_stereo", "zero_information",
         "some_zero_information", "exact_zero", "behind_camera", "ur_zero")
assert sorted(SPECS) == sorted(FROZEN + ADDED)
# the reference's iteration and trial counts are the same under all N_PERM summation orders.  fxfy_mono is not listed: none of its 400 seeds keeps
# its counts under every order (at its first seed they range over 21 .. 32 iterations), and it has no directed property to carry
DIRECTED = ("all_outliers_round", "inlier_again", "ten_rejections", "n3", "n9", "n10") + tuple(n for n in ADDED if n != "fxfy_mono")


def _rot(w):
    th = float(np.linalg.norm(w))
    if th == 0:
        return np.eye(3)
    k = np.asarray(w, np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _scene(seed, n, kind="mixed", outliers=0.15, start_scale=1.0, noise_scale=1.0, rot=None, cam=CAM):
    """-> (Tcw, cam, edges, details): details holds what an edited scene needs — the true pose as float32, the gross outliers' indices, the offset
    of every observation from the projection (noise and gross error) and which edges are stereo"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = cam
    Rt = _rot(rng.normal(0, 0.2, 3)) if rot is None else _rot(np.asarray(rot, np.float64))
    tt = rng.normal(0, 1.0, 3)
    u = rng.uniform(40, WIDTH - 40, n)
    v = rng.uniform(40, HEIGHT - 40, n)
    z = rng.uniform(2.0, 25.0, n)
    Pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    Xw = ((Pc - tt) @ Rt).astype(np.float32)                   # Rt^T (Pc - tt)
    Ttrue = np.eye(4)
    Ttrue[:3, :3], Ttrue[:3, 3] = Rt, tt
    Ttrue = Ttrue.astype(np.float32)
    pc = Xw.astype(np.float64) @ Ttrue[:3, :3].astype(np.float64).T + Ttrue[:3, 3].astype(np.float64)
    level = rng.integers(0, 8, n)
    s = 1.2 ** level
    noise = rng.normal(0, 0.6, (n, 3)) * s[:, None] * noise_scale
    uo = fx * pc[:, 0] / pc[:, 2] + cx + noise[:, 0]
    vo = fy * pc[:, 1] / pc[:, 2] + cy + noise[:, 1]
    uro = fx * pc[:, 0] / pc[:, 2] + cx - bf / pc[:, 2] + noise[:, 2]
    n_out = int(round(outliers * n))
    bad = rng.permutation(n)[:n_out]
    ang = rng.uniform(0, 2 * np.pi, n_out)
    mag = rng.uniform(20, 120, n_out)
    gross = np.zeros((n, 3))
    gross[bad] = np.stack([mag * np.cos(ang), mag * np.sin(ang), rng.uniform(-40, 40, n_out)], 1)
    uo[bad] += gross[bad, 0]
    vo[bad] += gross[bad, 1]
    uro[bad] += gross[bad, 2]
    stereo = {"mono": np.zeros(n, bool), "stereo": np.ones(n, bool), "mixed": rng.random(n) < 0.6}[kind]
    e = np.zeros(n, R.EDGE_DTYPE)
    e["Xw"], e["u"], e["v"] = Xw, uo, vo
    e["ur"] = np.where(stereo, np.maximum(uro, 0.0), -1.0)
    e["inv_sigma2"] = R.inv_sigma2((31.0 * s).astype(np.float32))
    e["kp"] = np.sort(rng.permutation(4 * n + 8)[:n])          # ascending keypoint indices with gaps
    T0 = np.eye(4)
    T0[:3, :3] = _rot(rng.normal(0, 0.005, 3) * start_scale) @ Ttrue[:3, :3].astype(np.float64)
    T0[:3, 3] = Ttrue[:3, 3].astype(np.float64) + rng.normal(0, 0.03, 3) * start_scale
    details = dict(Ttrue=Ttrue, bad=np.sort(bad), offset=noise + gross, stereo=stereo, size=(31.0 * s).astype(np.float32))
    return (Ttrue if start_scale == 0 else T0.astype(np.float32)), np.array(cam, np.float32), e, details


def scene(seed, n, kind="mixed", outliers=0.15, start_scale=1.0, noise_scale=1.0, rot=None, cam=CAM):
    """-> (Tcw float32 (4, 4) start pose, cam float32 [5], edges EDGE_DTYPE [n]).  rot: the true rotation as an axis-angle vector in place of the
    N(0, 0.2) draw (the generator's later draws do not move: the three normals are simply not taken); cam: (fx, fy, cx, cy, bf)"""
    return _scene(seed, n, kind, outliers, start_scale, noise_scale, rot, cam)[:3]


def _observe(e, idx, T, cam, offset, stereo):
    """rewrite the observations of edges idx as the projection of their points under pose T (float32 values, double arithmetic) plus offset"""
    fx, fy, cx, cy, bf = cam
    T = np.asarray(T, np.float32).astype(np.float64)
    pc = e["Xw"][idx].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    u = fx * pc[:, 0] / pc[:, 2] + cx
    e["u"][idx], e["v"][idx] = u + offset[idx, 0], fy * pc[:, 1] / pc[:, 2] + cy + offset[idx, 1]
    e["ur"][idx] = np.where(stereo[idx], np.maximum(u - bf / pc[:, 2] + offset[idx, 2], 0.0), -1.0)


def exact_problem():
    """identity pose, depths that are powers of two, coordinates with few bits: every projection is exact in float, every residual exactly zero"""
    fx, fy, cx, cy, bf = CAM
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
    return np.eye(4, dtype=np.float32), np.array(CAM, np.float32), e


N_SIGNED_ZERO = 3                                               # ur_zero: this many edges with ur = +0.0f and as many with -0.0f


def problem(name, seed):
    """-> (Tcw, cam, edges, aux) of case `name` at `seed`; aux: the edge indices a directed property speaks about"""
    n, kind, share, start, noise, want = SPECS[name]
    if want == "exact_zero":
        return exact_problem() + (None,)
    args = SCENE_ARGS.get(name, {})
    T, cam, e, d = _scene(seed, n, kind, share, start, noise, **args)
    camd = [float(c) for c in args.get("cam", CAM)]
    aux = None
    if want == "zero_information":
        e["inv_sigma2"] = 0.0
    elif want == "some_zero_information":
        aux = dict(zero=np.arange(0, n, 3), bad=d["bad"])
        e["inv_sigma2"][aux["zero"]] = 0.0
    elif want == "behind_camera":
        # X' = the point at -pc in the START pose's camera frame; observed from the true pose like every other point, so z < 0 and ur = u - bf / z
        aux = np.sort(np.random.default_rng(seed + 1).permutation(n)[:n // 5])
        T0 = T.astype(np.float64)
        pc = e["Xw"][aux].astype(np.float64) @ T0[:3, :3].T + T0[:3, 3]
        e["Xw"][aux] = (-pc - T0[:3, 3]) @ T0[:3, :3]
        _observe(e, aux, d["Ttrue"], camd, d["offset"], d["stereo"])
    elif want == "ur_zero":
        # points whose right-image column is 0 but for the noise (u = bf / z, z in 2 .. 2.1), observed with ur = +0.0f and -0.0f exactly
        rng = np.random.default_rng(seed + 1)
        aux = np.sort(rng.permutation(np.setdiff1d(np.arange(n), d["bad"]))[:2 * N_SIGNED_ZERO])
        fx, fy, cx, cy, bf = camd
        z = rng.uniform(2.0, 2.1, len(aux))
        Pc = np.stack([(bf / z - cx) / fx * z, (e["v"][aux].astype(np.float64) - cy) / fy * z, z], 1)
        Tt = d["Ttrue"].astype(np.float64)
        e["Xw"][aux] = (Pc - Tt[:3, 3]) @ Tt[:3, :3]
        d["stereo"][aux] = True
        _observe(e, aux, d["Ttrue"], camd, d["offset"], d["stereo"])
        e["ur"][aux[:N_SIGNED_ZERO]], e["ur"][aux[N_SIGNED_ZERO:]] = np.float32(0.0), np.float32(-0.0)
    return T, cam, e, aux


def quat_branch(m):
    """the branch Quat.from_matrix takes on rotation m: "trace", or 0 / 1 / 2 = the largest diagonal entry by Eigen's rule (ties keep the lower i)"""
    if m[0][0] + m[1][1] + m[2][2] > 0.0:
        return "trace"
    i = 1 if m[1][1] > m[0][0] else 0
    return 2 if m[2][2] > m[i][i] else i


def perms(n, count=N_PERM):
    return [np.random.default_rng(1000 + k).permutation(n) for k in range(count)]


def input_holds(want, T, e, aux):
    """the directed properties that the inputs alone decide"""
    m = np.asarray(T, np.float32).astype(np.float64)[:3, :3]
    if want in ("branch_i0", "branch_i1", "branch_i2"):
        return quat_branch(m) == int(want[-1])
    if want == "tie":
        return quat_branch(m) in (0, 1) and abs(m[0][0] - m[1][1]) <= 1e-3
    if want == "ur_zero":
        ur = e["ur"][aux]
        return bool((ur == 0).all() and not np.signbit(ur[:N_SIGNED_ZERO]).any() and np.signbit(ur[N_SIGNED_ZERO:]).all())
    return True


def result_holds(want, ref, T, e, aux):
    """the directed properties of the reference's result"""
    n = len(e)
    if want == "empty_round":
        return bool(ref["empty_rounds"])
    if want == "inlier_again":
        return bool(((ref["round_flags"][0] == 1) & (ref["outlier"] == 0)).any())
    if want == "ten_rejections":
        return ref["max_trials"] == 10
    if want == "zero_information":                              # 4 rounds of one iteration of 10 failed factorisations; nothing moves, nothing is an outlier
        return ((ref["rounds"], ref["lm_iterations"], ref["lm_trials"], ref["n_good"]) == (4, 4, 40, n) and not ref["round_flags"].any()
                and ref["Tcw_d"].tobytes() == R.se3_from_pose(T).matrix().tobytes())
    if want == "some_zero_information":                         # chi2 = 0 <= th whatever the residual: gross outliers among the zero weights stay inliers
        return not ref["outlier"][aux["zero"]].any() and len(np.intersect1d(aux["zero"], aux["bad"])) > 0 and bool(ref["outlier"].any())
    if want == "exact_zero":
        return (ref["rounds"], ref["lm_iterations"], ref["lm_trials"], ref["n_good"]) == (4, 4, 4, n)
    if want == "behind_camera":
        return bool((ref["outlier"][aux] == 0).any() and (ref["outlier"][aux] == 1).any())
    return True


def qualify(T, cam, e, want=None, fixed_path=False, aux=None, spread_cap=None):
    """-> (reference result, spread) or None.  spread: the largest deviation of Tcw_d under the permutations from the result in g2o's order"""
    if not input_holds(want, T, e, aux):
        return None
    ref = R.pose_optimization_fast(T, cam, e)
    if ref["status"] != R.STATUS_OK or not ref["min_margin"] >= MARGIN:
        return None
    if not result_holds(want, ref, T, e, aux):
        return None
    spread = 0.0
    for p in perms(len(e)):
        r = R.pose_optimization_fast(T, cam, e, sum_order=p)
        if not r["min_margin"] >= MARGIN or r["round_flags"].shape != ref["round_flags"].shape or not np.array_equal(r["round_flags"], ref["round_flags"]):
            return None
        if fixed_path and (r["lm_iterations"], r["lm_trials"]) != (ref["lm_iterations"], ref["lm_trials"]):
            return None                                         # a directed case's path is the same under every order
        spread = max(spread, float(np.abs(r["Tcw_d"] - ref["Tcw_d"]).max()))
    if spread_cap is not None and spread > spread_cap:
        return None                                             # tau is derived from the spread: a new case never widens it
    return ref, spread


def base_seed(name):
    return 7919 * (FROZEN.index(name) + 1) if name in FROZEN else 1000003 * (ADDED.index(name) + 1)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(T, cam, edges, ref, spread, seed, aux) of the first qualifying seed"""
    base = base_seed(name)
    for seed in range(base, base + 400):
        T, cam, e, aux = problem(name, seed)
        q = qualify(T, cam, e, SPECS[name][5], name in DIRECTED, aux, None if name in FROZEN else SPREAD_CAP)
        if q is not None:
            return dict(T=T, cam=cam, edges=e, ref=q[0], spread=q[1], seed=seed, aux=aux)
    raise AssertionError("no qualifying seed for " + name)


CHAIN_N = 2049                                                  # two chunks of hs_pose_edges_device's 1024 keypoints and one keypoint more
CHAIN_SEED = 1000003 * 100                                      # qualifies like a case: tests/test_poseopt_ref.py checks it on the CPU


@functools.lru_cache(maxsize=None)
def chain_problem():
    """A frame of CHAIN_N keypoints that all hold a landmark, for the chain hs_pose_edges_device -> hs_pose_optimize_device: a scene's edges taken
    apart into keypoints (x, y, size), uR, landmark positions in a shuffled order and the association.  -> dict(T, cam, kps, uR, kp_lm, lm_pos,
    edges): edges is the list the reference gathers from the arrays."""
    T, cam, e, d = _scene(CHAIN_SEED, CHAIN_N, "mixed", 0.15)
    e["kp"] = np.arange(CHAIN_N)
    kps = np.zeros(CHAIN_N, [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])   # hs_keypoint
    kps["x"], kps["y"], kps["size"] = e["u"], e["v"], d["size"]
    kp_lm = np.random.default_rng(CHAIN_SEED + 1).permutation(CHAIN_N).astype(np.int32)
    lm_pos = np.zeros((CHAIN_N, 3), np.float32)
    lm_pos[kp_lm] = e["Xw"]
    return dict(T=T, cam=cam, kps=kps, uR=e["ur"].copy(), kp_lm=kp_lm, lm_pos=lm_pos, edges=e)


EDGE_FRAME_SIZES = (1023, 1024, 1025, 2048, 2049, 3000)        # keypoint counts around hs_pose_edges_device's chunks of EDGE_CHUNK keypoints
EDGE_FRAME_VARIANTS = ("sparse", "gap", "all")
EDGE_CHUNK, EDGE_FRAME_L = 1024, 500


def edge_frame(n, variant):
    """Synthetic arrays for the edge gather, no extraction: -> dict(kps hs_keypoint [n] (x, y and a size of 8 pyramid levels), uR float32 [n], kp_lm
    int32 [n], lm_pos float32 (EDGE_FRAME_L, 3)).  "sparse": about half of the keypoints hold a landmark, the last keypoint of the first chunk and
    the first of the second do, and some entries are -1, INT32_MIN, L and L + 7 in either chunk; "gap": the same with one whole chunk holding
    nothing (the second of three, else the first); "all": every keypoint holds one."""
    rng = np.random.default_rng(5000 + n)
    L = EDGE_FRAME_L
    kps = np.zeros(n, [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])
    kps["x"], kps["y"] = rng.uniform(0, WIDTH, n), rng.uniform(0, HEIGHT, n)
    kps["size"] = (31.0 * 1.2 ** rng.integers(0, 8, n)).astype(np.float32)
    uR = np.where(rng.random(n) < 0.6, rng.uniform(0, 1, n) * kps["x"], -1.0).astype(np.float32)
    lm_pos = rng.normal(0, 5.0, (L, 3)).astype(np.float32)
    kp_lm = np.where(rng.random(n) < 0.5, rng.integers(0, L, n), -1).astype(np.int32)
    if variant == "all":
        kp_lm = rng.integers(0, L, n).astype(np.int32)
    else:
        for i, v in ((7, np.iinfo(np.int32).min), (311, L), (640, L + 7), (900, -1), (1030, L), (1500, np.iinfo(np.int32).min), (2040, L + 7), (2050, -1)):
            if i < n:
                kp_lm[i] = v
        for i in (0, EDGE_CHUNK - 1, EDGE_CHUNK, n - 1):
            if i < n:
                kp_lm[i] = (i * 37) % L
        if variant == "gap":
            c = 1 if n > 2 * EDGE_CHUNK else 0
            kp_lm[c * EDGE_CHUNK:(c + 1) * EDGE_CHUNK] = -1
    return dict(kps=kps, uR=uR, kp_lm=kp_lm, lm_pos=lm_pos)


def too_few(n):
    T, cam, e = scene(31 + n, max(n, 1), "mixed", 0.0)
    return T, cam, e[:n]


REF_KEYS = ("Tcw_d", "Tcw", "outlier", "n_edges", "n_good", "rounds", "lm_iterations", "lm_trials", "status")


def golden_arrays():
    """every case's inputs and reference outputs as the flat dict stored in GOLDEN, with the measured spread and the tolerance tau derived from it"""
    out, spread = {}, 0.0
    for name in sorted(SPECS):
        c = case(name)
        out[name + ".T"], out[name + ".cam"], out[name + ".edges"] = c["T"], c["cam"], c["edges"]
        for k in REF_KEYS:
            out[name + "." + k] = np.asarray(c["ref"][k])
        spread = max(spread, c["spread"])
    out["spread"] = np.float64(spread)
    out["tau"] = np.float64(TAU_FACTOR * spread)
    return out


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":                                      # python tests/poseopt_cases.py: rewrite tests/golden/poseopt_cases.npz
    arrays = golden_arrays()
    np.savez_compressed(GOLDEN, **arrays)
    print("%s: %d cases, spread %.3e, tau %.3e" % (GOLDEN, len(SPECS), float(arrays["spread"]), float(arrays["tau"])))
