"""Directed and seeded cases for the monocular initialisation (tests/test_monoinit_ref.py and tests/test_monoinit_abi.py on the CPU,
tests/test_gpu_monoinit*.py on the device).

A scene is seeded 3-D points in front of camera 1, projected into camera 1 and into a camera 2 that has moved by a known (R, t), with seeded pixel
noise, some matches replaced by gross outliers, and unmatched key points mixed into both frames, so that n1 != n2 and both exceed N and the matched
key points are neither the first nor contiguous.  Everything is built from hyslam_amd.synth.splitmix64 with + - * / and sqrt on float64
elementwise, so the same bytes come out on every machine.

A case: dict(kps1 [n1, 2] float32, kps2 [n2, 2] float32, matches12 [n1] int32, params, draws or None, expect: the status the scene is built to give
or None).  EXEMPT names the cases that sit on an edge on purpose: they are compared with LITERAL only.
"""
import functools

import numpy as np

import ref_monoinit as R
from hyslam_amd.synth import splitmix64

W, H_ = 640.0, 480.0
CAM = dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0)
# chunk sizes of hyslam_amd/csrc/hs_monoinit.h
KEY_CHUNK, CHI_CHUNK, RANK_CHUNK = 1024, 256, 1024
RANK_SEED = {-1: 60, 0: 60, 1: 62}                                 # RANSAC seeds of the rank_chunk cases, chosen so that the qualification holds
# n8, n9: every sample holds (nearly) every match, so several hypotheses score the same and the FIRST of them wins
EXEMPT = ("identical_points", "both_scores_zero", "n7_too_few", "two_motions_tie", "pure_rotation", "n8", "n9")


def uniform(seed, n, stream):
    return (splitmix64(seed, n, stream) >> np.uint64(11)).astype(np.float64) / float(1 << 53)


def rotation(seed, scale):
    q = np.concatenate([[1.0], (uniform(seed, 3, 300) - 0.5) * scale])
    w, x, y, z = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def project(X):
    return np.stack([CAM["fx"] * X[:, 0] / X[:, 2] + CAM["cx"], CAM["fy"] * X[:, 1] / X[:, 2] + CAM["cy"]], 1)


def scene(seed, N, kind="general", outliers=0.0, noise=0.3, extra1=None, extra2=None, t=(0.4, 0.05, 0.1), rot=0.1):
    """-> (kps1 [n1, 2], kps2 [n2, 2], matches12 [n1]).  kind: general (depths 3 .. 9), plane (one tilted plane), rotation (t = 0)"""
    u, v = (uniform(seed, N, 301) - 0.5) * 1.0, (uniform(seed, N, 302) - 0.5) * 0.75
    if kind == "plane":
        z = 5.0 / (1.0 - 0.16 * u - 0.1 * v)                    # the plane z = 5 + 0.16 x + 0.1 y
    else:
        z = 3.0 + 6.0 * uniform(seed, N, 303)
    X = np.stack([u * z, v * z, z], 1)
    Rm = rotation(seed, rot)
    tt = np.zeros(3) if kind == "rotation" else np.array(t, np.float64)
    X2 = np.stack([Rm[i, 0] * X[:, 0] + Rm[i, 1] * X[:, 1] + Rm[i, 2] * X[:, 2] + tt[i] for i in range(3)], 1)
    p1 = project(X) + (np.stack([uniform(seed, N, 304), uniform(seed, N, 305)], 1) - 0.5) * 2.0 * noise
    p2 = project(X2) + (np.stack([uniform(seed, N, 306), uniform(seed, N, 307)], 1) - 0.5) * 2.0 * noise
    out = uniform(seed, N, 308) < outliers
    wild = np.stack([uniform(seed, N, 309) * W, uniform(seed, N, 310) * H_], 1)
    p2 = np.where(out[:, None], wild, p2)
    e1 = N // 3 + 2 if extra1 is None else extra1
    e2 = N // 2 + 5 if extra2 is None else extra2
    return assemble(seed, p1, p2, e1, e2)


def assemble(seed, p1, p2, e1, e2):
    """mixes e1 / e2 unmatched key points into the frames at seeded places and permutes frame 2"""
    N = len(p1)
    n1, n2 = N + e1, N + e2
    k1 = np.stack([uniform(seed, n1, 311) * W, uniform(seed, n1, 312) * H_], 1)
    k2 = np.stack([uniform(seed, n2, 313) * W, uniform(seed, n2, 314) * H_], 1)
    place1 = np.sort(np.argsort(uniform(seed, n1, 315), kind="stable")[:N])
    place2 = np.argsort(uniform(seed, n2, 316), kind="stable")[:N]
    k1[place1], k2[place2] = p1, p2
    m = np.full(n1, -1, np.int32)
    m[place1] = place2
    return k1.astype(np.float32), k2.astype(np.float32), m


def word(place, avail):
    return ((place << 32) + avail - 1) // avail


def table(rows, N):
    """draws [len(rows), 8]: row = the eight PLACES drawn (from N, N - 1, ... available)"""
    d = np.zeros((len(rows), R.DRAW_STRIDE), np.uint32)
    for i, r in enumerate(rows):
        d[i] = [word(p, N - k) for k, p in enumerate(r)]
    return d


def case(sc, params=None, draws=None, expect=None):
    p = dict(R.DEFAULT)
    p.update(CAM)
    p.update(params or {})
    return dict(kps1=sc[0], kps2=sc[1], matches12=sc[2], params=p, draws=draws, expect=expect)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["general_f"] = case(scene(11, 150), dict(seed=3), expect=R.OK_F)
    c["plane_h"] = case(scene(12, 150, "plane", t=(0.5, 0.1, 0.05)), dict(seed=21), expect=R.OK_H)
    c["pure_rotation"] = case(scene(13, 120, "rotation"), dict(seed=5), expect=R.FAILED)
    c["outliers_30"] = case(scene(14, 200, outliers=0.3, noise=0.2), dict(seed=8), expect=R.OK_F)
    # a plane seen frontally with a translation along the axis: the two physical solutions of the homography tie
    c["two_motions_tie"] = case(scene(15, 120, "plane", t=(0.0, 0.0, 0.5), rot=0.0), dict(seed=7), expect=None)
    k1 = np.full((40, 2), 100.0, np.float32)
    c["identical_points"] = case((k1, k1.copy(), np.arange(40, dtype=np.int32)), dict(seed=8, max_iterations=20), expect=R.FAILED)
    # matches that no model fits: every chi-square of every hypothesis above its threshold but for the sample's own
    c["both_scores_zero"] = case(scene(16, 9, outliers=1.0, extra1=3, extra2=2), dict(seed=9, max_iterations=5, sigma=1e-4), expect=None)
    c["n7_too_few"] = case(scene(17, 7), dict(seed=10), expect=R.TOO_FEW)
    for N in (8, 9, 63, 64, 65):
        c["n%d" % N] = case(scene(20 + N, N), dict(seed=N + (N == 63), max_iterations=65, min_triangulated=5), expect=None)
    for its in (1, 63, 64, 65, 200):
        c["its%d" % its] = case(scene(31, 80), dict(seed=119, max_iterations=its, min_triangulated=20), expect=None)
    c["min_tri_above_accepted"] = case(scene(32, 60), dict(seed=12, max_iterations=40, min_triangulated=500, min_frac_triangulated=0.5), expect=R.FAILED)
    c["min_tri_below_accepted"] = case(scene(32, 60), dict(seed=12, max_iterations=40, min_triangulated=10, min_frac_triangulated=0.5), expect=R.OK_F)
    for d in (-1, 0, 1):                                           # the LDS chunk edges: stage 2's chi-squares (N), stage 1's keys (n1, n2), stage 4's cosines (N)
        c["chi_chunk%+d" % d] = case(scene(40 + d, CHI_CHUNK + d, extra1=7, extra2=9, noise=0.2), dict(seed={-1: 40, 0: 41, 1: 44}[d], max_iterations=30), expect=R.OK_F)
        c["key_chunk%+d" % d] = case(scene(50 + d, 90, extra1=KEY_CHUNK + d - 90, extra2=KEY_CHUNK + 1 - d - 90), dict(seed=50, max_iterations=8), expect=None)
    for d in (-1, 0, 1):
        c["rank_chunk%+d" % d] = case(scene(60 + d, RANK_CHUNK + d, extra1=3, extra2=3, noise=0.2), dict(seed=RANK_SEED[d], max_iterations=6), expect=R.OK_F)
    sc = scene(61, 40)
    c["directed_draws"] = case(sc, dict(seed=1, max_iterations=6), draws=table([[0, 1, 2, 3, 4, 5, 6, 7], [39, 38, 37, 36, 35, 34, 33, 32], [0, 0, 0, 0, 0, 0, 0, 0],
                                                                                  [39, 0, 37, 0, 35, 0, 33, 0]], 40), expect=None)
    return c


SWEEP_SEED = 9000


@functools.lru_cache(maxsize=None)
def sweep():
    """32 small seeded scenes: N in [8, 72), every kind, outliers up to 30 %"""
    out = {}
    for i in range(32):
        u = uniform(SWEEP_SEED + i, 6, 320)
        N = 8 + int(u[0] * 64)
        kind = ("general", "general", "plane", "rotation")[int(u[1] * 4)]
        out["sweep%02d" % i] = case(scene(SWEEP_SEED + 100 + i, N, kind, outliers=0.3 * u[2], noise=0.1 + 0.4 * u[3]),
                                    dict(seed=int(u[4] * 1e6), max_iterations=10 + int(u[5] * 30), min_triangulated=3 + N // 8), expect=None)
    return out


def batch_q3():
    c = cases()
    return [c["outliers_30"], c["n7_too_few"], c["plane_h"]]


def run_reference(c, kind="literal"):
    return R.estimate(c["kps1"], c["kps2"], c["matches12"], c["params"], c["draws"], kind)
