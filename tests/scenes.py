"""Synthetic tracking scenes for the matcher tests (BASELINE config 4 in miniature): a frame with extracted features and a
local map of landmarks back-projected from those features at seeded depths under a slightly different pose."""
import numpy as np

import oracle
from hyslam_amd.synth import synth_stereo_pair


def small_rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(np.float32)


def projection_scene(seed, w=640, h=480, nfeat=1000, copies=3, sensor=1, fx=500.0):
    """-> dict(frame_args=..., lms=LM array, kps, desc, uR).  frame_args feed oracle.make_frame_view(cls, **frame_args)."""
    rng = np.random.default_rng(seed)
    L, R = synth_stereo_pair(seed, w, h)
    p = oracle.default_params(nfeat)
    sp = oracle.stereo_params(fx=fx, mbf=fx * 0.12, n_rows=h)
    kps, desc, kR, dR, uR, depth = oracle.stereo_frontend(p, sp, L, R)
    n = len(kps)
    cx, cy = w / 2.0 - 0.5, h / 2.0 - 0.5
    Rcw = small_rotation(*(rng.normal(0, 0.004, 3)))
    tcw = rng.normal(0, 0.02, 3).astype(np.float32)
    Rwc = Rcw.T
    Ow = -Rwc @ tcw
    lms = np.zeros(n * copies + 40, oracle.LM_DTYPE)
    k = 0
    for c in range(copies):
        d = np.where(depth > 0, depth, rng.uniform(2.0, 25.0, n)).astype(np.float32) * rng.uniform(0.97, 1.03, n).astype(np.float32)
        px = kps["x"] + rng.normal(0, 1.5 if c else 0.3, n)
        py = kps["y"] + rng.normal(0, 1.5 if c else 0.3, n)
        Pc = np.stack([(px - cx) * d / fx, (py - cy) * d / fx, d], 1)
        Pw = (Rwc @ (Pc - tcw).T).T
        sl = slice(k, k + n)
        lms["pos"][sl] = Pw.astype(np.float32)
        lms["size"][sl] = (kps["size"] * d / fx * rng.uniform(0.7, 1.4, n)).astype(np.float32)
        dist = np.linalg.norm(Pw - Ow, axis=1)
        lms["min_dist"][sl] = (dist * rng.uniform(0.3, 1.1, n)).astype(np.float32)       # some fail the 0.8*min test
        lms["max_dist"][sl] = (dist * rng.uniform(0.9, 3.0, n)).astype(np.float32)       # some fail the 1.2*max test
        nrm = (Pw - Ow) / dist[:, None]                                 # mean viewing direction: camera -> point (MapPoint::UpdateNormalAndDepth)
        lms["normal"][sl] = nrm.astype(np.float32)
        dd = desc.copy()
        flips = rng.integers(0, 30 if c else 8, n)
        for i in range(n):
            bits = rng.integers(0, 256, flips[i])
            for b in bits:
                dd[i, b >> 3] ^= 1 << (b & 7)
        lms["desc"][sl] = dd
        lms["assoc_kp"][sl] = -1
        lms["prev_angle"][sl] = (kps["angle"] + rng.normal(0, 4, n) + (rng.random(n) < 0.1) * rng.uniform(0, 360, n)) % 360
        k += n
    # outliers: behind the camera, far outside the image, null entries
    t = lms[k:]
    t["pos"] = rng.normal(0, 30, (len(t), 3)).astype(np.float32)
    t["pos"][:10, 2] = -np.abs(t["pos"][:10, 2]) - 1
    t["size"], t["min_dist"], t["max_dist"], t["assoc_kp"] = 0.2, 0.1, 1e3, -1
    t["desc"] = rng.integers(0, 256, (len(t), 32), dtype=np.uint8)
    t["skip"][-5:] = 1
    # a few landmarks already associated with a keypoint of this frame (landMarkSizePixels uses the keypoint size then)
    pick = rng.choice(n, min(25, n), replace=False)
    lms["assoc_kp"][pick] = pick
    kp_lm_obs = np.full(n, -1, np.int32)
    kp_lm_obs[rng.choice(n, min(60, n), replace=False)] = rng.integers(0, 4, min(60, n))                  # 0 observations must NOT block a keypoint
    perm = rng.permutation(len(lms))
    frame_args = dict(Rcw=Rcw, tcw=tcw, fx=fx, fy=fx, cx=cx, cy=cy, mbf=fx * 0.12, sensor=sensor, bounds=(0.0, float(w), 0.0, float(h)),
                      kps=kps, desc=desc, uR=uR, kp_lm_obs=kp_lm_obs)
    return dict(frame_args=frame_args, lms=lms[perm].copy(), kps=kps, desc=desc, uR=uR)


def synthetic_featvec(desc, n_nodes, seed):
    """A seeded stand-in for DBoW2's FeatureVector (node id -> ascending keypoint indices): descriptors are hashed onto
    `n_nodes` vocabulary nodes by their first bits, so two views of the same point mostly share a node."""
    rng = np.random.default_rng(seed)
    sel = rng.choice(256, 12, replace=False)
    bits = np.unpackbits(desc, axis=1, bitorder="little")[:, sel]
    node = (bits.astype(np.int64) * (1 << np.arange(12))).sum(1) % n_nodes
    ids = np.unique(node)
    idx = np.concatenate([np.nonzero(node == i)[0] for i in ids]).astype(np.int32)
    ptr = np.concatenate([[0], np.cumsum([(node == i).sum() for i in ids])]).astype(np.int32)
    return ids.astype(np.int32) * 7 + 3, ptr, idx          # non-contiguous node ids, like real vocabulary node ids


# ---------------------------------------------------------------- stereo matcher edge cases
STEREO_EDGE_KINDS = ("boundaries", "bands", "clip", "disparity", "octaves", "ties", "thresholds", "median", "mixed")
# (th_high, th_low): the reference's 100/50, acceptance thresholds that are not integers (75.5, 62.5, 153.5), every distance below
# th_high (257) with everything accepted (256.5)
STEREO_THRESHOLDS = ((100.0, 50.0), (100.0, 51.0), (80.0, 50.0), (80.0, 45.0), (257.0, 50.0), (257.0, 256.0), (80.0, 79.0))


def flip_bits(rng, desc, k):
    """desc (n, 32) uint8 with exactly k[i] distinct bits of row i flipped: Hamming distance k[i] to the input."""
    n = len(desc)
    k = np.broadcast_to(np.asarray(k, np.int64), (n,))
    if n == 0:
        return desc.copy()
    rank = np.argsort(rng.random((n, 256)), 1).argsort(1)
    return np.bitwise_xor(desc, np.packbits(rank < k[:, None], axis=1, bitorder="little"))


def _edge_rows(rng, n, n_rows, kind):
    """y values: on and beside 32-row strip boundaries, fractional rows, negative rows, the last row, rows at and past n_rows"""
    H = max(n_rows, 1)
    on_strip = 32.0 * rng.integers(0, H // 32 + 2, n) + rng.choice([-1.0, -0.001, 0.0, 0.5, 31.5, -0.5], n)
    inside = rng.uniform(0, H, n)
    last = H - rng.choice([1.0, 0.5, 0.001, 1e-4], n)
    neg = -rng.choice([0.25, 1.0, 2.5, 17.0, 40.0], n)
    past = H + rng.choice([0.0, 0.25, 1.0, 16.0, 33.0], n)
    w = {"clip": [1, 2, 2, 2, 2], "boundaries": [5, 2, 1, 0.3, 0.3]}.get(kind, [2, 4, 1, 0.3, 0.3])
    pick = rng.choice(5, n, p=np.array(w) / sum(w))
    y = np.choose(pick, [on_strip, inside, last, neg, past])
    y[(y < 0) & (pick < 3)] = 0.0
    y[rng.random(n) < 0.02] = -0.0
    return y.astype(np.float32)


def stereo_edge_lists(rng, kind, nL=None, nR=None, n_rows=None, size_ref=None, th=None, fx=None):
    """Left and right keypoint lists with descriptors for the stereo matcher, aimed at one family of edges (`kind`, one of
    STEREO_EDGE_KINDS).  Most right keypoints are made from a left keypoint with a chosen row offset, disparity, octave step and
    Hamming distance (the left descriptor with exactly that many bits flipped); the others are unrelated.  The right list is shuffled,
    so equal distances turn up in any index order.  Returns (kL, dL, kR, dR, params), params being pyref.stereo_match's keyword
    arguments besides the lists.  Arguments left at None are drawn from the kind's ranges."""
    from oracle import KP_DTYPE
    f = np.float32
    nL = int(rng.integers(1, 400)) if nL is None else nL
    nR = int(rng.integers(1, 500)) if nR is None else nR
    if n_rows is None:
        n_rows = int(rng.choice([0, 1, 33, 100, 480] if kind == "clip" else [1, 33, 480, 1080, 1087]))
    if size_ref is None:
        size_ref = float(rng.choice({"bands": [7.5, 4.0, 2.0, 1e6], "ties": [4.0, 7.5], "boundaries": [31.0, 7.5, 4.0]}.get(kind, [31.0, 31.0, 7.5, 4.0, 1e6])))
    if th is None:
        th = (100.0, 50.0) if kind in ("median", "ties") else STEREO_THRESHOLDS[int(rng.integers(len(STEREO_THRESHOLDS)))]
    th_high, th_low = th
    if fx is None:
        fx = float(rng.choice([5.0, 5.25, 500.0, 1050.0, 1e5] if kind in ("disparity", "mixed") else [500.0, 1050.0]))
    mbf = float(f(fx) * f(rng.choice([0.12, 0.5, 0.07])))
    params = dict(fx=fx, mbf=mbf, n_rows=n_rows, th_high=th_high, th_low=th_low, size_ref=size_ref)
    max_d = f(f(mbf) / f(f(mbf) / f(fx)))
    accept = (f(th_high) + f(th_low)) / f(2)
    W = float(min(max(640.0, 2.5 * float(max_d)), 4000.0))

    # left keypoints
    kL = np.zeros(nL, KP_DTYPE)
    kL["y"] = _edge_rows(rng, nL, n_rows, kind)
    kL["octave"] = rng.integers(0, 8, nL)
    kL["size"] = f(31) * f(1.2) ** kL["octave"].astype(f)
    x = rng.uniform(0, W, nL)
    whole = rng.random(nL) < 0.3
    x[whole] = np.floor(x[whole])
    x[rng.random(nL) < 0.03] = -rng.choice([0.5, 2.0], 1)[0]          # maxU < 0: no search
    kL["x"] = x
    kL["angle"] = rng.uniform(0, 360, nL)
    kL["response"] = rng.integers(20, 90, nL)
    dL = rng.integers(0, 256, (nL, 32), dtype=np.uint8)
    if kind == "disparity":
        # Sterbenz: for uL in [maxD, 2 maxD] the subtraction uL - maxD is exact, so uR = uL - maxD gives a disparity of exactly maxD
        sel = rng.random(nL) < 0.4
        kL["x"][sel] = (max_d * f(1) + f(rng.uniform(0, 1, int(sel.sum()))) * max_d).astype(f)

    # right keypoints: made from a left one (src >= 0) or unrelated (src = -1)
    kR = np.zeros(nR, KP_DTYPE)
    src = rng.integers(0, max(nL, 1), nR) if nL else np.full(nR, -1)
    src[rng.random(nR) < (0.15 if kind != "mixed" else 0.4)] = -1
    if kind == "ties" and nL:
        # a few left keypoints get several right partners at one distance, each with a row band over the left row but in its own strip
        for iL in rng.choice(nL, max(1, min(nL, nR // 8)), replace=False):
            src[rng.choice(nR, min(nR, int(rng.integers(2, 6))), replace=False)] = iL
    own = src >= 0
    s = np.where(own, src, 0)
    octave = np.where(own, kL["octave"][s] if nL else 0, rng.integers(0, 8, nR))
    steps = {"octaves": [-2, -1, 1, 2, 0]}.get(kind, [0, 0, 0, 1, -1, 2, -2])
    octave = np.where(own, octave + rng.choice(steps, nR), octave)
    kR["octave"] = octave
    kR["size"] = f(31) * f(1.2) ** kR["octave"].astype(f)
    odd = rng.random(nR) < 0.1
    kR["size"][odd] = rng.uniform(0.5, 120.0, int(odd.sum()))
    r = f(2) * kR["size"] / f(size_ref)
    yL = kL["y"][s] if nL else np.zeros(nR, f)
    off = np.choose(rng.integers(0, 5, nR), [np.zeros(nR), rng.uniform(-1, 1, nR) * r, np.ceil(r) * rng.choice([-1, 1], nR),
                                              rng.uniform(-3, 3, nR) * r, rng.choice([-0.5, 0.5, 31.0, -32.0, 1.0], nR)])
    if kind == "ties":
        off = np.where(own, rng.uniform(-0.95, 0.95, nR) * np.maximum(r - 1, 0), off)
    kR["y"] = np.where(own, yL + off, _edge_rows(rng, nR, n_rows, kind)).astype(f)
    uL = kL["x"][s] if nL else np.zeros(nR, f)
    disp = np.choose(rng.choice(6, nR, p=[0.5, 0.15, 0.1, 0.1, 0.1, 0.05] if kind == "disparity" else [0.8, 0.05, 0.05, 0.04, 0.03, 0.03]),
                     [rng.uniform(0, max_d, nR).astype(f), np.zeros(nR, f), np.full(nR, max_d, f), max_d * f(1.001) + f(0.5) + np.zeros(nR, f),
                      rng.uniform(0, 1, nR).astype(f), -rng.uniform(0.5, 5, nR).astype(f)])
    xr = (uL - disp).astype(f)
    ulp = rng.random(nR) < (0.1 if kind == "disparity" else 0.02)
    xr[ulp] = np.nextafter(uL[ulp], f(np.inf))                      # one ulp right of uL: outside the window
    kR["x"] = np.where(own, xr, rng.uniform(0, W, nR)).astype(f)
    kR["angle"] = rng.uniform(0, 360, nR)
    kR["response"] = rng.integers(20, 90, nR)

    # distances
    if kind == "thresholds":
        ah, al = int(np.floor(accept)), int(np.ceil(accept))
        pool = [int(th_high), int(th_high) - 1, ah, al, ah - 1, 0, 3]
        k = rng.choice(pool, nR)
    elif kind == "median":
        m = int(rng.integers(2, 30))
        lo, hi = int(np.floor(f(2.1) * f(m))), int(np.ceil(f(1.5) * f(1.4) * f(m)))
        k = np.choose(rng.choice(4, nR, p=[0.45, 0.2, 0.2, 0.15]), [rng.integers(0, m + 1, nR), np.full(nR, lo), np.full(nR, hi), rng.integers(0, 80, nR)])
    elif kind == "ties":
        k = np.full(nR, int(rng.integers(5, 40)))
    else:
        k = np.choose(rng.choice(3, nR, p=[0.6, 0.3, 0.1]), [rng.integers(0, 60, nR), rng.integers(0, 257, nR), rng.integers(int(accept) - 2, int(accept) + 2, nR)])
    k = np.clip(k, 0, 256)
    dR = np.where(own[:, None], flip_bits(rng, dL[s] if nL else np.zeros((nR, 32), np.uint8), k), rng.integers(0, 256, (nR, 32), dtype=np.uint8))
    perm = rng.permutation(nR)
    return kL, dL, kR[perm].copy(), np.ascontiguousarray(dR[perm]), params
