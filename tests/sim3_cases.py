"""Directed and seeded cases for the batched Horn Sim3 RANSAC (tests/test_sim3_ref.py on the CPU, tests/test_gpu_sim3.py on the device).

A scene is points in front of camera 2 (X2c) and their images under a known similarity in camera 1's frame (X1c = s R X2c + t) with seeded noise of
a tenth of a millimetre, some of the matches replaced by gross outliers.  Everything is built from hyslam_amd.synth.splitmix64 with + - * / and sqrt
on float64 elementwise, so the same bytes come out on every machine.

QUALIFICATION (qualify).  For every hypothesis a case evaluates and every correspondence, both |err1 - threshold1| and |err2 - threshold2| exceed
MARGIN.  MARGIN is 8 x the largest difference, measured on the CPU over all cases, between the float err that LITERAL's pose gives and the float64
err at the same pose (ref_sim3.errors against ref_sim3.errors64), taken over the pairs whose float64 err is below NEAR: the largest threshold of any
case is 27 (9.210 x 2.9859 truncated), so no err at or above NEAR = 64 is within reach of a threshold whatever its rounding, and the rounding of a
far outlier's err (1e4 px^2 and more, rounding 1e-3 and more) says nothing about a decision.  Measured: 6.0e-4 (tests/test_sim3_ref.py prints it and
asserts that MARGIN covers 8 x it).  tests/test_sim3_ref.py ASSERTS the qualification for every case; it is never a filter, and no case is left
out: the seeds below were chosen on the CPU so that it holds.  The cases of EXEMPT sit on a threshold or on an acceptance edge on purpose; they are
exempt BY NAME and compared with the D19 reference only.
"""
import functools

import numpy as np

import ref_sim3 as R
from hyslam_amd.synth import splitmix64

NEAR = 64.0
MARGIN = 5e-3                    # >= 8 x the measured 6.0e-4 (module docstring)
K1 = tuple(np.float32(v) for v in (520.0, 515.0, 320.5, 240.25))
K2 = tuple(np.float32(v) for v in (458.0, 457.5, 367.25, 248.5))
SIGMA2 = (1.0, 1.44, 2.0736, 2.985984)                            # 1.2^(2 level)
EXEMPT = ("equal_counts_last_wins", "count_equals_min", "sigma_1_44", "err_equals_threshold", "collinear_sample", "duplicate_sample", "identical_sets")


def uniform(seed, n, stream):
    """n float64 in [0, 1) from the counter-based generator of hyslam_amd.synth"""
    return (splitmix64(seed, n, stream) >> np.uint64(11)).astype(np.float64) / float(1 << 53)


def similarity(seed):
    """(s, R, t): a rotation of a few tenths of a radian from a seeded unit quaternion (sqrt and division only), s in [0.8, 1.25), t in +-0.5"""
    q = np.concatenate([[1.0], (uniform(seed, 3, 190) - 0.5) * 0.6])
    w, x, y, z = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return 0.8 + 0.45 * uniform(seed, 1, 191)[0], Rm, uniform(seed, 3, 192) - 0.5


def scene(seed, N, outliers=0.3, noise=1e-4, fix_scale=False, sigma2=None):
    """corrs CORR_DTYPE [N].  outliers: a fraction (seeded choice) or an explicit index list."""
    s, Rm, t = similarity(seed)
    if fix_scale:
        s = 1.0
    X2 = np.stack([(uniform(seed, N, 193) - 0.5) * 4.0, (uniform(seed, N, 194) - 0.5) * 3.0, 3.0 + uniform(seed, N, 195) * 6.0], 1)
    X1 = np.stack([s * (Rm[i, 0] * X2[:, 0] + Rm[i, 1] * X2[:, 1] + Rm[i, 2] * X2[:, 2]) + t[i] for i in range(3)], 1)
    X1 = X1 + (np.stack([uniform(seed, N, 196 + i) for i in range(3)], 1) - 0.5) * 2.0 * noise
    if isinstance(outliers, float):
        out = uniform(seed, N, 199) < outliers
    else:
        out = np.zeros(N, bool)
        out[list(outliers)] = True
    wild = np.stack([(uniform(seed, N, 200) - 0.5) * 4.0, (uniform(seed, N, 201) - 0.5) * 3.0, 3.0 + uniform(seed, N, 202) * 6.0], 1)
    X1 = np.where(out[:, None], wild, X1)
    c = np.zeros(N, R.CORR_DTYPE)
    c["X1c"], c["X2c"] = X1.astype(np.float32), X2.astype(np.float32)
    lv = (uniform(seed, N, 203) * 4).astype(np.int64) if sigma2 is None else np.zeros(N, np.int64)
    lw = (uniform(seed, N, 204) * 4).astype(np.int64) if sigma2 is None else np.zeros(N, np.int64)
    tab = np.array(SIGMA2 if sigma2 is None else (sigma2,), np.float32)
    c["sigma2_1"], c["sigma2_2"] = tab[lv], tab[lw]
    c["idx1"] = np.arange(N) * 2 + 1                               # the matches the constructor skipped leave gaps
    return c


def word(place, avail):
    """a draws entry that the reduction (w * avail) >> 32 maps to `place`"""
    return ((place << 32) + avail - 1) // avail


def table(rows, N):
    """draws [len(rows), DRAW_STRIDE]: row = the three PLACES drawn (from N, N - 1, N - 2 available)"""
    d = np.zeros((len(rows), R.DRAW_STRIDE), np.uint32)
    for i, r in enumerate(rows):
        d[i, :3] = [word(p, N - k) for k, p in enumerate(r)]
    return d


def case(corrs, params=None, draws=None, calls=(5,), k1=K1, k2=K2):
    return dict(corrs=corrs, params=dict(R.DEFAULT, **(params or {})), draws=draws, calls=tuple(calls), k1=k1, k2=k2)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    # seeded: both scale modes, two different cameras, the LoopClosing parameters
    c["n100"] = case(scene(11, 100), dict(seed=5), calls=(300,))
    c["n100_rounds"] = case(scene(12, 100, outliers=0.7), dict(seed=6), calls=(5, 5, 5))          # a state carried over three calls of 5
    c["n40_fix_scale"] = case(scene(13, 40, fix_scale=True), dict(seed=7, fix_scale=1, min_inliers=10), calls=(20,))
    c["n30_same_camera"] = case(scene(14, 30), dict(seed=8, min_inliers=8), calls=(12,), k2=K1)
    c["n100_sparse"] = case(scene(34, 100, outliers=0.85), dict(seed=34), calls=(300,))          # 20 inliers at the most, 20 > 20 fails: all 300 run
    c["n257"] = case(scene(15, 257), dict(seed=9), calls=(7,))                                   # one past the LDS staging chunk
    # the gates
    c["n3_min3"] = case(scene(16, 3, outliers=[]), dict(min_inliers=3, seed=1), calls=(5,))      # N = min_inliers = 3: one iteration, 3 > 3 fails
    c["n3_min2"] = case(scene(16, 3, outliers=[]), dict(min_inliers=2, seed=1), calls=(5,))
    c["n3_min0"] = case(scene(16, 3, outliers=[]), dict(min_inliers=0, seed=1), calls=(5,))
    c["n_equals_min"] = case(scene(17, 12, outliers=[]), dict(min_inliers=12, seed=2), calls=(5, 5))      # one iteration, then an exhausted state
    c["too_few"] = case(scene(17, 11, outliers=[]), dict(min_inliers=12, seed=2), calls=(5,))
    c["n2_min0"] = case(scene(18, 2, outliers=[]), dict(min_inliers=0, seed=3), calls=(5,))
    c["n0"] = case(scene(18, 0, outliers=[]), dict(min_inliers=0, seed=3), calls=(5,))
    # acceptance edges: 8 inliers (0 .. 7) and 12 gross outliers, min_inliers = 8: a count of 8 equals min_inliers and must not return; the first three
    # rows draw three inlier triples, so 8, 8, 8 come in a row and the LAST one is the state's best
    eq = scene(19, 20, outliers=list(range(8, 20)), noise=0.0)
    c["equal_counts_last_wins"] = case(eq, dict(min_inliers=8, seed=4), table([(0, 1, 2), (3, 4, 5), (1, 6, 2)], 20), calls=(3,))
    c["count_equals_min"] = case(eq, dict(min_inliers=8, seed=4), table([(0, 1, 2)], 20), calls=(1, 4))
    c["exhausted_state"] = case(scene(20, 10, outliers=[7, 8, 9]), dict(min_inliers=9, seed=4), calls=(300, 5, 5))
    # thresholds: sigma2 = 1.44 gives 13, not 13.26: correspondence 9 misses its own image by sqrt(13.1) pixels in u
    th = scene(21, 10, outliers=[], noise=0.0, sigma2=1.44)
    th["X1c"][9, 0] += np.float32(np.sqrt(13.1) * float(th["X1c"][9, 2]) / float(K1[0]))
    c["sigma_1_44"] = case(th, dict(min_inliers=3, seed=4), table([(0, 1, 2)], 10), calls=(1,))
    # err equal to the threshold: correspondence 9 misses by (3, 2) pixels, and five float steps further in x its err1 is 13.0f exactly (found by a
    # search over float steps on the CPU; tests/test_sim3_ref.py asserts the equality): 13 < 13 fails, an outlier
    eq13 = scene(21, 10, outliers=[], noise=0.0, sigma2=1.44)
    z9 = float(eq13["X1c"][9, 2])
    bx = np.float32(eq13["X1c"][9, 0] + np.float32(3.0 * z9 / 520.0))
    eq13["X1c"][9, 1] = np.float32(eq13["X1c"][9, 1] + np.float32(2.0 * z9 / 515.0))
    eq13["X1c"][9, 0] = (bx.view(np.int32) + np.int32(5)).view(np.float32)
    c["err_equals_threshold"] = case(eq13, dict(min_inliers=3, seed=4), table([(0, 1, 2)], 10), calls=(1,))
    # depth: z = 0 on either side (non-finite image: an outlier) and a point behind both cameras that the similarity maps consistently (an inlier:
    # nothing checks the sign of z)
    z = scene(22, 16, outliers=[], noise=0.0)
    z["X1c"][13, 2] = 0.0
    z["X2c"][14, 2] = 0.0
    s, Rm, t = similarity(22)
    behind = np.array([0.3, -0.2, -4.0])
    z["X2c"][15] = behind.astype(np.float32)
    z["X1c"][15] = (s * (Rm @ z["X2c"][15].astype(np.float64)) + t).astype(np.float32)
    c["z_zero_or_negative"] = case(z, dict(min_inliers=5, seed=4), table([(0, 1, 2), (13, 1, 2), (14, 1, 2), (15, 1, 2)], 16), calls=(4,))
    # degenerate samples
    same = scene(23, 12, outliers=[], noise=0.0)
    same["X1c"] = same["X2c"]
    c["identical_sets"] = case(same, dict(min_inliers=0, seed=4), calls=(5,))
    col = scene(24, 12, outliers=[], noise=0.0)
    for k in (1, 2):
        col["X2c"][k] = col["X2c"][0] + np.float32(k) * np.array([0.25, 0.5, 0.125], np.float32)
        col["X1c"][k] = col["X1c"][0] + np.float32(k) * np.array([0.5, 0.25, -0.125], np.float32)
    c["collinear_sample"] = case(col, dict(min_inliers=3, seed=4), table([(0, 1, 2)], 12), calls=(2,))
    # the sampler's quirk, N = 12.  Places (0, 0, 9): the first draw takes value 0 and writes avail[0] = 11; the second draws place 0 again, takes 11 and
    # writes avail[11] = avail.back(), a place popped already: no effect; the third takes 9.  Places (5, 5, 5): values 5, 11 and, since avail[5] is
    # still 11, 11 again: the same point twice.
    c["popped_slot"] = case(scene(25, 12, outliers=[]), dict(min_inliers=3, seed=4), table([(0, 0, 9)], 12), calls=(1,))
    c["duplicate_sample"] = case(scene(25, 12, outliers=[]), dict(min_inliers=3, seed=4), table([(5, 5, 5)], 12), calls=(1,))
    return c


def solver(cs, **kw):
    return R.Solver(cs["corrs"], cs["k1"], cs["k2"], cs["params"], cs["draws"], **kw)


def run(cs, **kw):
    """every call of the case on one solver: (results, solver)"""
    s = solver(cs, **kw)
    return [s.iterate(n) for n in cs["calls"]], s


def all_hypotheses(cs, rotation="d19"):
    """(a, b) of every hypothesis the case's calls could evaluate, whether or not an earlier one returns"""
    s = solver(cs, rotation=rotation)
    if s.N < 3 or s.N < s.min_inliers:
        return None
    n = min(s.max_its, sum(cs["calls"]))
    _, _, _, _, a, b, _ = s.hypotheses(0, n)
    return a, b


def qualify(cs):
    """the smallest |err - threshold| over every hypothesis and correspondence of the case (inf where nothing is finite)"""
    ab = all_hypotheses(cs)
    if ab is None:
        return np.inf
    e1, e2 = R.errors(ab[0], ab[1], cs["corrs"], np.asarray(cs["k1"], np.float32), np.asarray(cs["k2"], np.float32))
    with np.errstate(all="ignore"):
        d = np.concatenate([np.abs(R.D(e1) - R.D(R.threshold(cs["corrs"]["sigma2_1"]))[None]).reshape(-1),
                            np.abs(R.D(e2) - R.D(R.threshold(cs["corrs"]["sigma2_2"]))[None]).reshape(-1)])
    d = d[np.isfinite(d)]
    return float(d.min()) if len(d) else np.inf


def rounding(cs):
    """the largest |float err - float64 err| at LITERAL's poses over the pairs with a float64 err below NEAR"""
    ab = all_hypotheses(cs, rotation="literal")
    if ab is None:
        return 0.0
    k1, k2 = np.asarray(cs["k1"], np.float32), np.asarray(cs["k2"], np.float32)
    worst = 0.0
    for ef, ed in zip(R.errors(ab[0], ab[1], cs["corrs"], k1, k2), R.errors64(ab[0], ab[1], cs["corrs"], k1, k2)):
        with np.errstate(all="ignore"):
            near = np.isfinite(ed) & (ed < NEAR) & np.isfinite(ef)
            if near.any():
                worst = max(worst, float(np.abs(R.D(ef) - ed)[near].max()))
    return worst
