"""Inputs of the pose-only optimisation tests (tests/test_poseopt_ref.py, tests/test_gpu_poseopt.py): seeded generators and directed cases.

A scene is a camera like the bench's (fx = fy = 700, 1280x720, bf = 84), points 2..25 units in front of a true pose, a start pose a few cm / ~0.5
degrees off, keypoint sizes 31 * 1.2^level, pixel noise scaled by the level and a chosen share of gross outliers.  Every input is rounded to
float32, as the C ABI carries it.

A case QUALIFIES when, in the reference (ref_poseopt.pose_optimization_fast), every classification of every round has |chi2/th - 1| >= MARGIN and
the flags of all rounds are identical under N_PERM seeded summation orders.  A generator draws the next seed until its case qualifies and any
directed property holds (`want`), so what a name stands for is fixed by this file alone.  tests/golden/poseopt_cases.npz holds the inputs and the
reference's outputs of every case; the GPU tests read only that file."""
import functools
import os

import numpy as np

import ref_poseopt as R

CAM = (700.0, 700.0, 640.0, 360.0, 84.0)
WIDTH, HEIGHT = 1280, 720
MARGIN, N_PERM, TAU_FACTOR = 1e-4, 8, 16
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
DIRECTED = ("all_outliers_round", "inlier_again", "ten_rejections", "n3", "n9", "n10")
BATCH = ("batch_257", None, "batch_12")                         # Q = 3 with sizes (257, 0, 12); None = a problem without edges
TOO_FEW = (0, 2)                                                # edge counts below 3: not optimised


def _rot(w):
    th = float(np.linalg.norm(w))
    if th == 0:
        return np.eye(3)
    k = np.asarray(w, np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def scene(seed, n, kind="mixed", outliers=0.15, start_scale=1.0, noise_scale=1.0):
    """-> (Tcw float32 (4, 4) start pose, cam float32 [5], edges EDGE_DTYPE [n])"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = CAM
    Rt, tt = _rot(rng.normal(0, 0.2, 3)), rng.normal(0, 1.0, 3)
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
    uo[bad] += mag * np.cos(ang)
    vo[bad] += mag * np.sin(ang)
    uro[bad] += rng.uniform(-40, 40, n_out)
    stereo = {"mono": np.zeros(n, bool), "stereo": np.ones(n, bool), "mixed": rng.random(n) < 0.6}[kind]
    e = np.zeros(n, R.EDGE_DTYPE)
    e["Xw"], e["u"], e["v"] = Xw, uo, vo
    e["ur"] = np.where(stereo, np.maximum(uro, 0.0), -1.0)
    e["inv_sigma2"] = R.inv_sigma2((31.0 * s).astype(np.float32))
    e["kp"] = np.sort(rng.permutation(4 * n + 8)[:n])          # ascending keypoint indices with gaps
    T0 = np.eye(4)
    T0[:3, :3] = _rot(rng.normal(0, 0.005, 3) * start_scale) @ Ttrue[:3, :3].astype(np.float64)
    T0[:3, 3] = Ttrue[:3, 3].astype(np.float64) + rng.normal(0, 0.03, 3) * start_scale
    return (Ttrue if start_scale == 0 else T0.astype(np.float32)), np.array(CAM, np.float32), e


def perms(n, count=N_PERM):
    return [np.random.default_rng(1000 + k).permutation(n) for k in range(count)]


def qualify(T, cam, e, want=None, fixed_path=False):
    """-> (reference result, spread) or None.  spread: the largest deviation of Tcw_d under the permutations from the result in g2o's order"""
    ref = R.pose_optimization_fast(T, cam, e)
    if ref["status"] != R.STATUS_OK or not ref["min_margin"] >= MARGIN:
        return None
    if want == "empty_round" and not ref["empty_rounds"]:
        return None
    if want == "inlier_again" and not ((ref["round_flags"][0] == 1) & (ref["outlier"] == 0)).any():
        return None
    if want == "ten_rejections" and ref["max_trials"] != 10:
        return None
    spread = 0.0
    for p in perms(len(e)):
        r = R.pose_optimization_fast(T, cam, e, sum_order=p)
        if not r["min_margin"] >= MARGIN or r["round_flags"].shape != ref["round_flags"].shape or not np.array_equal(r["round_flags"], ref["round_flags"]):
            return None
        if fixed_path and (r["lm_iterations"], r["lm_trials"]) != (ref["lm_iterations"], ref["lm_trials"]):
            return None                                         # a directed case's path is the same under every order
        spread = max(spread, float(np.abs(r["Tcw_d"] - ref["Tcw_d"]).max()))
    return ref, spread


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(T, cam, edges, ref, spread, seed) of the first qualifying seed"""
    n, kind, share, start, noise, want = SPECS[name]
    base = 7919 * (sorted(SPECS).index(name) + 1)
    for seed in range(base, base + 400):
        T, cam, e = scene(seed, n, kind, share, start, noise)
        q = qualify(T, cam, e, want, name in DIRECTED)
        if q is not None:
            return dict(T=T, cam=cam, edges=e, ref=q[0], spread=q[1], seed=seed)
    raise AssertionError("no qualifying seed for " + name)


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
