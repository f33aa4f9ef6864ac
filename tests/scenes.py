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


# ---------------------------------------------------------------- grid-area matchers: edge cases
AREA_BOUNDS = ((0.0, 640.0, 0.0, 480.0), (32.0, 608.0, 16.0, 464.0), (13.5, 627.25, 7.75, 471.0), (0.0, 64.0, 0.0, 48.0))
AREA_KINDS = ("mixed", "cell_edges", "bounds", "nonfinite", "crowded", "radius", "ties", "landmark_edges")


def _area_frame(rng, n, bounds, fx=512.0, identity=True):
    """a keyframe with n uniformly placed keypoints and random descriptors; identity pose (exact projections) or a small rotation"""
    from oracle import KP_DTYPE
    minx, maxx, miny, maxy = bounds
    k = np.zeros(n, KP_DTYPE)
    k["x"] = rng.uniform(minx, maxx, n); k["y"] = rng.uniform(miny, maxy, n)
    k["size"] = rng.choice([7.0, 15.5, 31.0, 44.6], n); k["angle"] = rng.uniform(0, 360, n); k["response"] = rng.random(n)
    k["octave"] = rng.integers(0, 8, n)
    Rcw = np.eye(3, dtype=np.float32) if identity else small_rotation(*rng.normal(0, 0.01, 3))
    tcw = np.zeros(3, np.float32) if identity else rng.normal(0, 0.05, 3).astype(np.float32)
    cx, cy = (minx + maxx) / 2, (miny + maxy) / 2
    return dict(Rcw=Rcw, tcw=tcw, fx=fx, fy=fx, cx=cx, cy=cy, mbf=fx * 0.1, sensor=1, bounds=bounds, kps=k,
                desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), uR=(k["x"] - rng.uniform(1, 40, n)).astype(np.float32),
                kp_lm_obs=rng.integers(-1, 3, n).astype(np.int32), size_ref=31.0)


def _area_landmarks(rng, fa, src, flips):
    """one landmark per keypoint index in src: back-projected at a seeded depth with the frame's pose, descriptor = the keypoint's with
    `flips` bits flipped, invariance range around its distance, normal along the viewing ray"""
    from oracle import LM_DTYPE
    f = np.float32
    k = fa["kps"][src]
    L = len(src)
    d = rng.uniform(1.0, 20.0, L)
    Pc = np.stack([(k["x"].astype(np.float64) - fa["cx"]) * d / fa["fx"], (k["y"].astype(np.float64) - fa["cy"]) * d / fa["fy"], d], 1)
    R, t = np.asarray(fa["Rcw"], np.float64), np.asarray(fa["tcw"], np.float64)
    with np.errstate(all="ignore"):
        Pw = (R.T @ (Pc - t).T).T
        Ow = -R.T @ t
        dist = np.linalg.norm(Pw - Ow, axis=1)
        lm = np.zeros(L, LM_DTYPE)
        lm["pos"] = Pw.astype(f)
        lm["size"] = (k["size"] * d / fa["fx"] * rng.uniform(0.7, 1.4, L)).astype(f)
        lm["min_dist"] = (dist * rng.uniform(0.3, 1.05, L)).astype(f)
        lm["max_dist"] = (dist * rng.uniform(0.95, 3.0, L)).astype(f)
        lm["normal"] = ((Pw - Ow) / dist[:, None]).astype(f)
    lm["desc"] = flip_bits(rng, fa["desc"][src], flips)
    lm["assoc_kp"] = -1
    lm["prev_angle"] = k["angle"]
    return lm


def _scw(fa, s):
    S = np.eye(4, dtype=np.float32)
    S[:3, :3] = np.float32(s) * np.asarray(fa["Rcw"], np.float32)
    S[:3, 3] = np.float32(s) * np.asarray(fa["tcw"], np.float32)
    return S


def _place_kps(rng, fa, kind):
    """overwrite keypoint coordinates of `fa` with the placements of one family of edges"""
    k = fa["kps"]
    n = len(k)
    if n == 0:
        return
    minx, maxx, miny, maxy = (np.float32(b) for b in fa["bounds"])
    cw, ch = (maxx - minx) / np.float32(64), (maxy - miny) / np.float32(48)
    m = max(1, n // 3)
    sel = rng.choice(n, min(m, n), replace=False)
    if kind == "cell_edges":
        # area-query cell edges (min + j*cw) and PosInGrid rounding edges (min + (j+0.5)*cw), exactly and one ulp either side
        jx = rng.integers(0, 65, len(sel)); jy = rng.integers(0, 49, len(sel))
        half = rng.choice([0.0, 0.5], len(sel))
        x = (minx + (jx + half) * cw).astype(np.float32); y = (miny + (jy + half) * ch).astype(np.float32)
        step = rng.choice([-1, 0, 1], (2, len(sel)))
        x = np.where(step[0] < 0, np.nextafter(x, np.float32(-np.inf)), np.where(step[0] > 0, np.nextafter(x, np.float32(np.inf)), x))
        y = np.where(step[1] < 0, np.nextafter(y, np.float32(-np.inf)), np.where(step[1] > 0, np.nextafter(y, np.float32(np.inf)), y))
        k["x"][sel], k["y"][sel] = x, y
    elif kind == "bounds":
        vx = np.array([minx, maxx, np.nextafter(maxx, np.float32(-np.inf)), np.nextafter(maxx, np.float32(np.inf)), minx - np.float32(1e-3),
                       np.nextafter(minx, np.float32(-np.inf)), maxx + 5, minx - 7, maxx - cw / 2, maxx - cw / 2 - np.float32(1e-3)], np.float32)
        vy = np.array([miny, maxy, np.nextafter(maxy, np.float32(-np.inf)), np.nextafter(maxy, np.float32(np.inf)), miny - np.float32(1e-3),
                       np.nextafter(miny, np.float32(-np.inf)), maxy + 5, miny - 7, maxy - ch / 2, maxy - ch / 2 - np.float32(1e-3)], np.float32)
        a, b = rng.integers(0, len(vx), len(sel)), rng.integers(0, len(vy), len(sel))
        keep = rng.random(len(sel)) < 0.4                                       # one coordinate on an edge, the other inside
        k["x"][sel] = np.where(keep, k["x"][sel], vx[a]); k["y"][sel] = np.where(keep, vy[b], k["y"][sel])
        k["x"][sel[keep]] = vx[a[keep]]
    elif kind == "nonfinite":
        v = np.array([np.nan, np.inf, -np.inf, 1e10, -1e10, 3e9, -0.0], np.float32)
        a = rng.integers(0, len(v), len(sel))
        which = rng.integers(0, 3, len(sel))
        k["x"][sel] = np.where(which != 1, v[a], k["x"][sel]); k["y"][sel] = np.where(which != 0, v[a], k["y"][sel])


def _area_case(rng, kind, n=None, L=None, bounds=None):
    f = np.float32
    bounds = AREA_BOUNDS[rng.integers(0, len(AREA_BOUNDS))] if bounds is None else bounds
    n = int(rng.integers(1, 400)) if n is None else n
    identity = kind in ("landmark_edges", "radius") or rng.random() < 0.5
    fa = _area_frame(rng, n, bounds, fx=float(rng.choice([512.0, 300.0, 1000.0])) if kind != "landmark_edges" else 512.0, identity=identity)
    minx, maxx, miny, maxy = (f(b) for b in bounds)
    cw, ch = (maxx - minx) / f(64), (maxy - miny) / f(48)
    th = int(rng.choice([1, 3, 4, 7, 10]))
    th_low = float(rng.choice([50, 64, 100]))
    if kind == "crowded" and n > 0:
        # m keypoints of one cell (everything else spread as usual): 0, 1, 64, 65, 300 or 5000 in the same mGrid list
        m = int(rng.choice([0, 1, 64, 65, 300, 5000]))
        from oracle import KP_DTYPE
        cxi, cyi = rng.integers(0, 64), rng.integers(0, 48)
        extra = np.zeros(m, KP_DTYPE)
        extra["x"] = minx + (cxi + rng.uniform(-0.45, 0.45, m)) * cw; extra["y"] = miny + (cyi + rng.uniform(-0.45, 0.45, m)) * ch
        extra["size"] = 31.0; extra["angle"] = rng.uniform(0, 360, m)
        base = fa["desc"][rng.integers(0, n, 1)][0]
        ed = flip_bits(rng, np.repeat(base[None], m, 0), rng.integers(0, 6, m))                 # many near-equal distances inside one cell
        pos = np.sort(rng.choice(n + m, m, replace=False))
        kk = np.insert(fa["kps"], pos - np.arange(m), extra)
        dd = np.insert(fa["desc"], pos - np.arange(m), ed, axis=0)
        fa.update(kps=kk, desc=dd, uR=np.insert(fa["uR"], pos - np.arange(m), extra["x"] - 5), kp_lm_obs=np.insert(fa["kp_lm_obs"], pos - np.arange(m), -1))
        n = n + m
    elif kind in ("cell_edges", "bounds", "nonfinite"):
        _place_kps(rng, fa, kind)
    elif kind == "mixed":
        _place_kps(rng, fa, str(rng.choice(["cell_edges", "bounds", "nonfinite"])))
    k = fa["kps"]
    L = int(rng.integers(0, 300)) if L is None else L
    src = rng.integers(0, max(n, 1), L) if n > 0 else np.zeros(L, np.int64)
    if n == 0:
        fa0 = _area_frame(rng, 1, bounds); src_fa = fa0
    else:
        src_fa = fa
    flips = rng.choice([0, 3, 20, int(th_low), int(th_low) + 1, 90], L)
    lms = _area_landmarks(rng, src_fa, src, flips)
    if L:
        dup = rng.random(L) < 0.15                                              # a copy of an earlier landmark competes for the same keypoint
        j = np.nonzero(dup)[0]; j = j[j > 0]
        lms[j] = lms[rng.integers(0, j, len(j))] if len(j) else lms[j]
        lms["skip"] = rng.random(L) < 0.08
        if n > 0:
            a = rng.random(L) < 0.2
            lms["assoc_kp"][a] = rng.integers(0, n, a.sum())
    if kind == "radius" and n > 0:
        # radii th * size / size_ref of 0, subnormal, one cell, the whole image, 3e10, +inf, negative and NaN: through the associated
        # keypoint's size, the landmark's own size (projected width) and th
        sizes = np.array([0.0, 1e-42, cw * f(31) / f(th), (maxx - minx) * f(31) / f(th), 3e10, np.inf, -5.0, np.nan], np.float32)
        hot = rng.choice(n, min(n, len(sizes)), replace=False)
        k["size"][hot] = sizes[:len(hot)]
        if L:
            a = rng.random(L) < 0.5
            lms["assoc_kp"][a] = rng.choice(hot, a.sum())
            b = ~a & (rng.random(L) < 0.5)
            lms["size"][b] = rng.choice(np.array([0.0, 1e-40, 1e30, np.inf, -1.0, np.nan], np.float32), b.sum())
        th = int(rng.choice([0, 1, 1, 2, 5]))
    if kind == "ties" and n > 0 and L > 0:
        # equal Hamming distances in different cells: B (lower index) is one cell right and one cell up of A, so column order, row order and index
        # order each pick a different winner
        from oracle import KP_DTYPE
        t = rng.choice(L, min(L, 20), replace=False)
        extra = np.zeros(2 * len(t), KP_DTYPE)
        dd = np.zeros((2 * len(t), 32), np.uint8)
        for q, li in enumerate(t):
            j = src[li]
            x0, y0 = k["x"][j], k["y"][j]
            extra[2 * q + 1]["x"], extra[2 * q + 1]["y"] = x0 - f(0.6) * cw, y0 + f(0.6) * ch           # A
            extra[2 * q]["x"], extra[2 * q]["y"] = x0 + f(0.6) * cw, y0 - f(0.6) * ch                   # B
            dd[2 * q] = dd[2 * q + 1] = lms["desc"][li]
        extra["size"] = 31.0
        fa.update(kps=np.concatenate([k, extra]), desc=np.concatenate([fa["desc"], dd]), uR=np.concatenate([fa["uR"], extra["x"] - 5]),
                  kp_lm_obs=np.concatenate([fa["kp_lm_obs"], np.full(len(extra), -1, np.int32)]))
        lms["assoc_kp"][t] = -1
        lms["size"][t] = np.float32(cw * 2.5 * fa["fx"] / 512)
        lms["skip"][t] = 0
        n = len(fa["kps"])
        th = max(th, 3)
    if kind == "landmark_edges" and L > 0:
        _landmark_edges(rng, fa, lms, th)
    kp_matched = (rng.random(n) < rng.choice([0.0, 0.1, 0.5])).astype(np.uint8)
    return dict(kind=kind, fa=fa, lms=lms, Scw=_scw(fa, rng.choice([1.0, 2.0, 0.37, 3.1])), th=th, th_low=th_low, kp_matched=kp_matched,
                window=int(rng.choice([0, 1, 10, 30, 100, 700, 1 << 30, 2147483647])))


def _landmark_edges(rng, fa, lms, th):
    """landmarks at camera z = +-0, exactly on the image bounds (IsInImage is strict above, Camera::Project inclusive), exactly at min_dist /
    max_dist and with PO.n exactly 0.5*dist.  Needs the identity pose: camera = world coordinates, projections exact."""
    f = np.float32
    minx, maxx, miny, maxy = (f(b) for b in fa["bounds"])
    fx, cx, cy = f(fa["fx"]), f(fa["cx"]), f(fa["cy"])
    L = len(lms)
    for i in rng.choice(L, min(L, 40), replace=False):
        which = rng.integers(0, 6)
        Z = f(rng.choice([1.0, 2.0, 4.0]))
        if which == 0:                                                          # z = +0 / -0
            lms["pos"][i] = [f(rng.uniform(-1, 1)), f(rng.uniform(-1, 1)), f(rng.choice([0.0, -0.0]))]
        elif which in (1, 2):                                                   # u or v exactly on a bound
            ux = [minx, maxx][rng.integers(0, 2)]; vy = [miny, maxy][rng.integers(0, 2)]
            X = f((ux - cx) / fx) * Z; Y = f((vy - cy) / fx) * Z
            if which == 1:
                Y = f(rng.uniform(-0.2, 0.2)) * Z
            lms["pos"][i] = [X, Y, Z]
            n = len(fa["kps"])
            if n:                                                               # a keypoint inside the grid, near the projection, with the landmark's
                j = rng.integers(0, n)                                          # descriptor: only the bound convention decides whether it matches
                u, v = cx + fx * (X / Z), cy + fx * (Y / Z)
                k = fa["kps"]
                k["x"][j] = u - 6 if u >= maxx else (u + 3 if u <= minx else u)
                k["y"][j] = v - 6 if v >= maxy else (v + 3 if v <= miny else v)
                k["size"][j] = 310.0                                           # radius th * 10 through assoc_kp
                fa["desc"][j] = lms["desc"][i]
                fa["uR"][j] = f(u - fa["mbf"] / Z)
                fa["kp_lm_obs"][j] = -1
                lms["assoc_kp"][i] = j
        else:
            lms["pos"][i] = [f(rng.uniform(-0.3, 0.3)) * Z, f(rng.uniform(-0.2, 0.2)) * Z, Z]
        p = lms["pos"][i].astype(np.float64)
        dist = f(np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]))
        if which == 3:                                                          # on the invariance range limits, or one ulp outside
            lms["min_dist"][i] = rng.choice([dist, np.nextafter(dist, f(np.inf))]); lms["max_dist"][i] = dist * f(2)
        elif which == 4:
            lms["max_dist"][i] = rng.choice([dist, np.nextafter(dist, f(-np.inf))]); lms["min_dist"][i] = dist * f(0.5)
        else:
            lms["min_dist"][i], lms["max_dist"][i] = dist * f(0.5), dist * f(2)
        if which == 5:                                                          # PO.n == 0.5*dist exactly (the reference rejects only dot < 0.5*dist)
            lms["pos"][i] = [0.0, 0.0, Z]
            lms["normal"][i] = [f(0.8660254), 0.0, rng.choice([f(0.5), np.nextafter(f(0.5), f(0))])]
            lms["min_dist"][i], lms["max_dist"][i] = Z * f(0.5), Z * f(2)
        lms["skip"][i] = 0


def area_sim3_pair(rng, case):
    """a second keyframe for SearchBySim3 from an area case: x_c1 = s12 R12 x_c2 + t12; KF2's keypoints are the landmarks' projections (jittered,
    shuffled, a few unrelated), lms1 / lms2 = the landmark of each keypoint of KF1 / KF2, assoc_kp pointing into the other keyframe"""
    f = np.float32
    fa = case["fa"]
    n1 = len(fa["kps"])
    s12 = float(rng.choice([1.0, 1.1, 1 / 1.1, 1e-3, 1e3, 0.37, 2.0]))
    R12 = small_rotation(*rng.normal(0, 0.003, 3))
    t12 = rng.normal(0, 0.02, 3).astype(f)
    src = _area_landmarks(rng, fa, np.arange(n1), rng.choice([0, 5, 20, 100], n1)) if n1 else case["lms"][:0].copy()
    R1, t1 = np.asarray(fa["Rcw"], np.float64), np.asarray(fa["tcw"], np.float64)
    R2 = (R12.T.astype(np.float64) @ R1).astype(f)
    t2 = ((R12.T.astype(np.float64) @ (t1 - t12)) / s12).astype(f)
    with np.errstate(all="ignore"):
        Pc2 = (R2.astype(np.float64) @ src["pos"].astype(np.float64).T).T + t2
        u = fa["fx"] * Pc2[:, 0] / Pc2[:, 2] + fa["cx"]; v = fa["fy"] * Pc2[:, 1] / Pc2[:, 2] + fa["cy"]
    n2 = int(rng.integers(max(n1 - 5, 0), n1 + 6)) if n1 else int(rng.integers(0, 3))
    fb = _area_frame(rng, n2, fa["bounds"], fx=fa["fx"])
    fb.update(Rcw=R2, tcw=t2, size_ref=fa["size_ref"])
    perm = rng.permutation(n2)
    m = min(n1, n2)
    with np.errstate(all="ignore"):
        fb["kps"]["x"][perm[:m]] = (u[:m] + rng.normal(0, 0.5, m)).astype(f)
        fb["kps"]["y"][perm[:m]] = (v[:m] + rng.normal(0, 0.5, m)).astype(f)
    fb["kps"]["size"][perm[:m]] = fa["kps"]["size"][:m]
    fb["desc"][perm[:m]] = flip_bits(rng, src["desc"][:m], rng.choice([0, 4, 30, 99, 100, 101], m))
    if rng.random() < 0.3:
        _place_kps(rng, fb, str(rng.choice(["cell_edges", "bounds", "nonfinite"])))
    lms1 = src.copy()
    lms2 = np.zeros(n2, lms1.dtype)
    lms2["skip"] = 1
    inv = np.full(n2, -1); inv[perm[:m]] = np.arange(m)
    own = inv >= 0
    lms2[own] = src[inv[own]]
    lms2["skip"][own] = rng.random(own.sum()) < 0.1
    lms2["desc"][own] = fb["desc"][own]
    lms1["skip"] = rng.random(n1) < 0.1
    lms1["assoc_kp"] = -1; lms2["assoc_kp"] = -1
    if n2:
        a = rng.random(n1) < 0.25; lms1["assoc_kp"][a] = rng.integers(0, n2, a.sum())
    if n1:
        a = rng.random(n2) < 0.25; lms2["assoc_kp"][a] = rng.integers(0, n1, a.sum())
    return dict(fb=fb, lms1=lms1, lms2=lms2, s12=s12, R12=R12, t12=t12, th=float(rng.choice([0.0, 1.0, 7.5, 15.0, 1e30])),
                th_high=float(rng.choice([99.0, 100.0])))


def area_edge_cases(seed):
    """Frames, landmarks and parameters for the grid-area queries: one case of every AREA_KINDS family, with keypoint and landmark counts
    drawn per case (the size extremes are in area_size_cases)."""
    rng = np.random.default_rng(seed)
    for kind in AREA_KINDS:
        case = _area_case(rng, kind)
        case["sim3"] = area_sim3_pair(rng, case)
        yield case


def area_size_cases(seed):
    """F.n of 0, 1 and 65 535 keypoints and L of 0, 1, 64, 65 and 20 000 landmarks"""
    rng = np.random.default_rng(seed)
    for n, L, kind in ((0, 5, "mixed"), (1, 1, "mixed"), (1, 0, "bounds"), (300, 64, "ties"), (300, 65, "radius"), (2000, 20000, "mixed"),
                       (65535, 200, "mixed"), (65535, 20000, "cell_edges")):
        case = _area_case(rng, kind, n=n, L=L)
        case["sim3"] = area_sim3_pair(rng, case)
        yield case


# ---------------------------------------------------------------- vocabulary-grouped matchers, vocabulary transform, 2-NN: edge cases
# Input domain of the reference (tests/ref_bow.py): angles finite in [0, 360), node ids ascending and unique, a feature index in at most one node.
BOW_KINDS = ("ties", "list_sizes", "single_candidate", "thresholds", "rotation_bins", "three_maxima", "epipolar", "competition",
             "disjoint_and_empty_nodes", "unsorted_lists", "mixed")
BOW_GPU_SEEDS = tuple(range(300, 312))         # the seeds the GPU test runs bow_edge_cases with; the CPU self-checks of the generators cover the same
BOW_PYREF_MAX_N = 2000                          # above this many features per side the oracle alone is the expectation
F12_RECTIFIED = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)         # pure x translation: l = (0, 1, -y1), dsqr = (y2 - y1)^2
# sigma_ref with size == size_ref for which 3.84 * sigma2 is exactly 9.0 in double (3.84 * 150 rounds to 576.0; 150 / 64 scales it exactly)
SIGMA_REF_BOUND_9 = 2.34375


def desc_bits(*set_bits):
    """the 32-byte descriptor with exactly these bits set"""
    m = np.zeros(256, np.uint8); m[list(set_bits)] = 1
    return np.packbits(m, bitorder="little")


def plain_kps(n, **fields):
    """n key points of size 31 and angle 0, named fields overwritten"""
    from oracle import KP_DTYPE
    k = np.zeros(n, KP_DTYPE)
    k["size"] = 31.0
    for name, v in fields.items():
        k[name] = v
    return k


def _bow_kps(rng, n):
    from oracle import KP_DTYPE
    k = np.zeros(n, KP_DTYPE)
    k["x"] = rng.uniform(0, 640, n); k["y"] = rng.uniform(0, 480, n)
    k["octave"] = rng.integers(0, 8, n)
    k["size"] = np.float32(31) * np.float32(1.2) ** k["octave"].astype(np.float32)
    k["angle"] = rng.uniform(0, 359.99, n); k["response"] = rng.integers(20, 90, n)
    return k


def _near(rng, base, k):
    """len(k) descriptors at exactly k[i] bits from `base` (32 bytes)"""
    k = np.atleast_1d(np.asarray(k, np.int64))
    return flip_bits(rng, np.repeat(np.asarray(base, np.uint8)[None, :], len(k), 0), k)


def _scatter_keep_order(rng, labels):
    """global index of every local slot: random, but ascending inside a label in local order (list position == local position)"""
    n = len(labels)
    slot = rng.permutation(n)
    g = np.empty(n, np.int64)
    g[np.lexsort((np.arange(n), labels))] = slot[np.lexsort((slot, labels))]
    return g


def _featvec_from_labels(labels, empty_ids=()):
    """CSR feature vector from a node label per feature (-1 = in no node): ids ascending, indices ascending per node; empty_ids = nodes that are
    present with an empty list"""
    labels = np.asarray(labels, np.int64)
    ids = np.unique(np.concatenate([labels[labels >= 0], np.asarray(empty_ids, np.int64)]))
    order = np.argsort(labels, kind="stable")
    order = order[labels[order] >= 0]
    counts = np.array([(labels == i).sum() for i in ids], np.int64) if len(ids) < 4096 else np.bincount(np.searchsorted(ids, labels[labels >= 0]), minlength=len(ids))
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return ids.astype(np.int32), ptr, order.astype(np.int32)


def _bow_finish(rng, kind, lab1, k1, d1, lab2, k2, d2, empty1=(), empty2=(), shuffle2=False, **params):
    """scatter the local (node, list position) arrays to global feature indices and add the case's parameters"""
    g1, g2 = _scatter_keep_order(rng, lab1), _scatter_keep_order(rng, lab2)
    K1, K2 = np.zeros_like(k1), np.zeros_like(k2)
    D1, D2 = np.zeros_like(d1), np.zeros_like(d2)
    L1, L2 = np.zeros_like(lab1), np.zeros_like(lab2)
    K1[g1], D1[g1], L1[g1] = k1, d1, lab1
    K2[g2], D2[g2], L2[g2] = k2, d2, lab2
    fv1, fv2 = _featvec_from_labels(L1, empty1), _featvec_from_labels(L2, empty2)
    if shuffle2:
        idx = fv2[2].copy()
        for j in range(len(fv2[0])):
            idx[fv2[1][j]:fv2[1][j + 1]] = rng.permutation(idx[fv2[1][j]:fv2[1][j + 1]])
        fv2 = (fv2[0], fv2[1], idx)
    case = dict(kind=kind, k1=K1, d1=D1, fv1=fv1, k2=K2, d2=D2, fv2=fv2, keep1=None, keep2=None, F12=None, size_ref=31.0, sigma_ref=1.0,
                score_threshold=50.0, ratio=0.8, check_rotation=int(rng.integers(0, 2)), host_only=bool(shuffle2))
    case.update(params)
    return case


class _BowBuilder:
    """collects nodes as local arrays: add(node id, side-1 descriptors, side-2 descriptors) -> (slice of side 1, slice of side 2)"""

    def __init__(self, rng):
        self.rng = rng
        self.lab1, self.lab2, self.d1, self.d2 = [], [], [], []
        self.n1 = self.n2 = 0
        self.empty1, self.empty2 = [], []

    def add(self, nid, d1, d2, on1=True, on2=True):
        d1 = np.asarray(d1, np.uint8).reshape(-1, 32); d2 = np.asarray(d2, np.uint8).reshape(-1, 32)
        s1, s2 = slice(self.n1, self.n1 + len(d1)), slice(self.n2, self.n2 + len(d2))
        self.lab1.append(np.full(len(d1), nid if on1 else -1)); self.lab2.append(np.full(len(d2), nid if on2 else -1))
        self.d1.append(d1); self.d2.append(d2)
        self.n1 += len(d1); self.n2 += len(d2)
        if on1 and len(d1) == 0:
            self.empty1.append(nid)
        if on2 and len(d2) == 0:
            self.empty2.append(nid)
        return s1, s2

    def related(self, nid, a, b, flips, unrelated=0.2, **kw):
        """a random side-1 descriptors; side 2: copies of them with a number of bits from `flips` flipped, or unrelated"""
        rng = self.rng
        d1 = rng.integers(0, 256, (a, 32), dtype=np.uint8)
        d2 = rng.integers(0, 256, (b, 32), dtype=np.uint8)
        if a and b:
            own = rng.random(b) >= unrelated
            src = rng.integers(0, a, b)
            d2 = np.where(own[:, None], flip_bits(rng, d1[src], rng.choice(flips, b)), d2)
        return self.add(nid, d1, d2, **kw)

    def arrays(self):
        cat = lambda x, w: np.concatenate(x) if x else np.zeros((0,) + w, np.uint8)
        lab1 = np.concatenate(self.lab1).astype(np.int64) if self.lab1 else np.zeros(0, np.int64)
        lab2 = np.concatenate(self.lab2).astype(np.int64) if self.lab2 else np.zeros(0, np.int64)
        return lab1, _bow_kps(self.rng, self.n1), cat(self.d1, (32,)), lab2, _bow_kps(self.rng, self.n2), cat(self.d2, (32,))

    def finish(self, kind, k1=None, k2=None, **params):
        lab1, K1, d1, lab2, K2, d2 = self.arrays()
        return _bow_finish(self.rng, kind, lab1, K1 if k1 is None else k1, d1, lab2, K2 if k2 is None else k2, d2,
                           empty1=self.empty1, empty2=self.empty2, **params)


def _node_ids(rng, n):
    return np.sort(rng.choice(np.arange(1, 40 * n + 50), n, replace=False)) * 3 + 1


def _bow_ties(rng):
    """equal best distances at different list positions (different lanes, and the same lane 64 apart), equal second-best, over lists up to 200"""
    B = _BowBuilder(rng)
    for nid in _node_ids(rng, int(rng.integers(3, 7))):
        a, b = int(rng.integers(1, 10)), int(rng.choice([2, 5, 66, 70, 130, 200]))
        d1 = rng.integers(0, 256, (a, 32), dtype=np.uint8)
        d2 = rng.integers(0, 256, (b, 32), dtype=np.uint8)
        free = list(rng.permutation(b))
        for r in range(a):
            t = int(rng.integers(2, 5))
            if len(free) < t + 1:
                break
            pos = [free.pop() for _ in range(t)]
            if b >= 66 and rng.random() < 0.5:                                  # two of them 64 apart: the same lane of the strided scan
                j = int(rng.integers(0, b - 64))
                if j in free and j + 64 in free:
                    free.remove(j); free.remove(j + 64); pos[:2] = [j, j + 64]
            k = int(rng.integers(0, 40))
            if rng.random() < 0.5:
                d2[pos] = _near(rng, d1[r], [k] * t)                              # tie on the best distance
            else:
                d2[pos] = _near(rng, d1[r], [k] + [k + int(rng.integers(1, 9))] * (t - 1))   # unique best, tie on the second
        B.add(nid, d1, d2)
    return B.finish("ties", ratio=float(rng.choice([0.8, 1.0, 1.5, 1.0])), score_threshold=float(rng.choice([50.0, 30.5])))


def _bow_list_sizes(rng):
    """side-2 lists of 0, 1, 63, 64, 65, 129 (the lanes stride by 64), side-1 lists that are not multiples of 4 (the waves stride by 4)"""
    B = _BowBuilder(rng)
    sizes2 = [0, 1, 63, 64, 65, 129]
    sizes1 = list(rng.permutation([0, 1, 2, 3, 5, 6, 7, 9]))
    for nid, b in zip(_node_ids(rng, len(sizes2)), rng.permutation(sizes2)):
        B.related(nid, int(sizes1.pop()), int(b), [0, 3, 10, 20, 49, 50], unrelated=0.5)
    return B.finish("list_sizes")


def _bow_single(rng):
    """exactly one candidate: bestDist2 stays FLT_MAX.  Through a list of one and through keep2 leaving one of many"""
    B = _BowBuilder(rng)
    for nid in _node_ids(rng, int(rng.integers(3, 8))):
        B.related(nid, int(rng.integers(1, 7)), int(rng.choice([1, 1, 7, 70])), [0, 5, 30, 49, 50, 60], unrelated=0.0)
    case = B.finish("single_candidate", ratio=float(rng.choice([0.5, 1e-30, 0.0, 1.0])))
    # keep2 leaves one feature of every longer side-2 list
    keep2 = np.ones(len(case["k2"]), np.uint8)
    ids, ptr, idx = case["fv2"]
    for j in range(len(ids)):
        lst = idx[ptr[j]:ptr[j + 1]]
        if len(lst) > 1:
            keep2[lst] = 0
            keep2[lst[int(rng.integers(0, len(lst)))]] = 1
    case["keep2"] = keep2
    return case


BOW_THRESHOLDS = (0.0, 0.5, 30.5, 50.0, 255.5, 256.0, 257.0, 1e30, np.inf, -1.0)
BOW_RATIOS = (0.0, 0.5, float(np.nextafter(np.float32(1), np.float32(0))), 1.0, float(np.nextafter(np.float32(1), np.float32(2))), 2.0, np.inf)


def _bow_thresholds(rng, thr=None, ratio=None):
    """best distances at and beside the score threshold, second-best at and beside best / ratio; fractional and extreme thresholds and ratios"""
    thr = float(rng.choice(BOW_THRESHOLDS)) if thr is None else thr
    ratio = float(rng.choice(BOW_RATIOS)) if ratio is None else ratio
    if thr > np.finfo(np.float32).max and ratio > 1:                              # outside the reference's domain
        ratio = 1.0
    t0 = int(np.clip(np.floor(thr) if np.isfinite(thr) else 256, 0, 256))
    B = _BowBuilder(rng)
    for nid in _node_ids(rng, int(rng.integers(3, 7))):
        a, b = int(rng.integers(1, 8)), int(rng.choice([3, 20, 70]))
        d1 = rng.integers(0, 256, (a, 32), dtype=np.uint8)
        d2 = rng.integers(0, 256, (b, 32), dtype=np.uint8)
        free = list(rng.permutation(b))
        for r in range(a):
            if len(free) < 2:
                break
            kb = int(np.clip(rng.choice([t0 - 1, t0, t0 + 1, 0, 10, 20]), 0, 256))
            ks = int(np.clip(rng.choice([kb, kb + 1, 2 * kb, 2 * kb + 1, 256]), kb, 256))
            d2[[free.pop(), free.pop()]] = _near(rng, d1[r], [kb, ks])
        B.add(nid, d1, d2)
    return B.finish("thresholds", score_threshold=thr, ratio=ratio)


def _rotation_pairs():
    f = np.float32
    n15l, n15h = np.nextafter(f(15), f(0)), np.nextafter(f(15), f(16))
    pairs = [(0, 15), (0, n15l), (0, n15h), (10, 25), (0, 45), (0, 75), (0, 345), (20, 5), (f(1e-6), 0), (0, 0), (f(359.99), 0), (0, f(359.99)),
             (100, 205), (15, 0), (n15h, 0), (345, 0), (0, f(1e-6)), (200, 95), (30, 60), (60, 30), (7.5, 22.5), (352.5, 7.5), (0, 14.999), (0, 15.001)]
    return np.array(pairs, f)


def _bow_rotation(rng, kind="rotation_bins", counts=None):
    """every pair at distance 0 in its own node (accepted by construction), angles chosen for the histogram.  rotation_bins: rot on a half bin
    (15, 45, ... degrees), one ulp beside, 0, 360 after the wrap; three_maxima: bin populations at the 10 % rule's boundary"""
    f = np.float32
    if counts is None:
        pool = _rotation_pairs()
        ang = pool[rng.integers(0, len(pool), int(rng.integers(40, 120)))]
        ang = np.concatenate([pool, ang])
    else:
        bins = rng.choice(12, len(counts), replace=False)                       # rot = 30 * bin exactly (angle1 = 0)
        ang = np.concatenate([np.tile(np.array([[0, 30.0 * b]], f), (c, 1)) for b, c in zip(bins, counts)] + [np.zeros((0, 2), f)])
        ang = ang[rng.permutation(len(ang))]
    n = len(ang)
    per = int(rng.choice([1, 3, n if n else 1]))
    ids = _node_ids(rng, max((n + per - 1) // per, 1))
    d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    lab = np.repeat(ids, per)[:n].astype(np.int64)
    k1, k2 = _bow_kps(rng, n), _bow_kps(rng, n)
    k1["angle"], k2["angle"] = ang[:, 0], ang[:, 1]
    return _bow_finish(rng, kind, lab, k1, d1, lab.copy(), k2, d1.copy(), check_rotation=1, ratio=0.8, score_threshold=50.0)


THREE_MAXIMA_COUNTS = ([10, 1], [10], [20, 2, 1], [20, 1, 1], [30, 3, 2], [30, 2, 3], [11, 1, 1], [19, 2, 1], [10, 10, 10, 10], [5, 5, 5, 5],
                       [40, 4, 3], [40, 3, 4], [1], [], [100, 10, 9, 9], [100, 9, 10])


def _bow_epipolar(rng, variant):
    """the epipolar gate: `bound` = rectified pair with dsqr exactly on, one ulp below and above 3.84 * sigma2; `den0` = lines with a = b = 0 for one
    keypoint (F maps it to the epipole) or for all (zero F); `nonfinite` = NaN / inf in F12 or in a keypoint"""
    f = np.float32
    B = _BowBuilder(rng)
    for nid in _node_ids(rng, int(rng.integers(2, 6))):
        B.related(nid, int(rng.integers(1, 9)), int(rng.choice([1, 4, 30, 70])), [0, 3, 10, 20, 40], unrelated=0.1)
    lab1, k1, d1, lab2, k2, d2 = B.arrays()
    n1, n2 = len(k1), len(k2)
    params = dict(check_rotation=int(rng.integers(0, 2)), ratio=1.0, score_threshold=90.0, keep1=(rng.random(n1) < 0.9).astype(np.uint8),
                  keep2=(rng.random(n2) < 0.9).astype(np.uint8))
    if variant == "bound":
        k1["y"] = np.where(rng.random(n1) < 0.5, 0.0, rng.integers(0, 400, n1)).astype(f)
        # one side-1 row per node decides the side-2 rows: y2 = y1 + dy, exact in float
        for nid in np.unique(lab1):
            i1 = np.nonzero(lab1 == nid)[0]; i2 = np.nonzero(lab2 == nid)[0]
            y1 = k1["y"][i1[rng.integers(0, len(i1), len(i2))]]
            big = rng.random(len(i2)) < 0.3                                       # size = 2 * size_ref: the bound is 36, dy = 6
            s = np.where(big, 2.0, 1.0).astype(f)
            dy0 = np.choose(rng.integers(0, 5, len(i2)), [f(3), np.nextafter(f(3), f(0)), np.nextafter(f(3), f(4)), f(0), f(1.5)])
            dyn = rng.choice(np.array([3.0, 2.5, 3.5, 0.0, -3.0, -2.5, -3.5], f), len(i2))
            k2["y"][i2] = np.where(y1 == 0, dy0 * s, y1 + dyn * s).astype(f)
            k2["size"][i2] = f(31) * s
        params.update(F12=F12_RECTIFIED.copy(), size_ref=31.0, sigma_ref=SIGMA_REF_BOUND_9)
    elif variant == "den0":
        if rng.random() < 0.3:
            F = np.zeros((3, 3), f); F[:, 2] = rng.normal(0, 1, 3)
        else:
            F = np.array([[1, 0, 0.01], [0, 1, -0.02], [-5, -7, 1]], f)           # a = x1 - 5, b = y1 - 7
            hit = rng.random(n1) < 0.4
            k1["x"][hit], k1["y"][hit] = 5.0, 7.0
        params.update(F12=F, sigma_ref=float(rng.choice([1.0, 1e4, 1e12])))
    else:
        F = (rng.normal(0, 1, (3, 3)) * np.array([[1e-5, 1e-5, 1e-2], [1e-5, 1e-5, 1e-2], [1e-2, 1e-2, 1.0]])).astype(f)
        which = int(rng.integers(0, 4))
        if which == 0:
            F[rng.integers(0, 3), rng.integers(0, 3)] = np.nan
        elif which == 1:
            F[rng.integers(0, 3), rng.integers(0, 3)] = rng.choice([np.inf, -np.inf])
        else:
            for k in (k1, k2):
                hit = rng.random(len(k)) < 0.25
                k["x"][hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30], f), hit.sum())
                hit = rng.random(len(k)) < 0.1
                k["y"][hit] = rng.choice(np.array([np.nan, np.inf], f), hit.sum())
            hit = rng.random(n2) < 0.2
            k2["size"][hit] = rng.choice(np.array([0.0, np.inf, np.nan, 1e30, -31.0], f), hit.sum())
        params.update(F12=F, sigma_ref=float(rng.choice([1.0, 4.0, 1e6])))
    return _bow_finish(rng, "epipolar", lab1, k1, d1, lab2, k2, d2, empty1=B.empty1, empty2=B.empty2, **params)


def _bow_competition(rng):
    """many side-1 features of one node are closest to the same few side-2 features, which sit at list positions around the 64-lane boundary:
    in the legacy matcher every step must see what the step before took"""
    B = _BowBuilder(rng)
    for nid in _node_ids(rng, int(rng.integers(1, 4))):
        a, b = int(rng.integers(20, 100)), int(rng.integers(66, 140))
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        d1 = _near(rng, base, rng.integers(0, 12, a))
        d2 = rng.integers(0, 256, (b, 32), dtype=np.uint8)
        good = np.unique(np.concatenate([[0, b - 1], rng.choice([62, 63, 64, 65, 66], 3, replace=False), rng.integers(0, b, 2)]))
        d2[good] = _near(rng, base, rng.integers(0, 14, len(good)))
        B.add(nid, d1, d2)
    return B.finish("competition", ratio=float(rng.choice([0.9, 1.0, 1.2])), score_threshold=50.0)


def _bow_disjoint(rng, variant=0):
    """node ids that only one side has, in runs (the merge walk jumps with lower_bound), shared nodes with an empty list on either side;
    variant 1: no node at all on side 2; variant 2: none on side 1"""
    B = _BowBuilder(rng)
    ids = _node_ids(rng, int(rng.integers(12, 30)))
    state = rng.choice(4, len(ids), p=[0.35, 0.25, 0.25, 0.15])                   # shared, side 1 only, side 2 only, shared with an empty list
    state[:4] = [1, 1, 0, 3]; state[-4:] = [2, 2, 2, 0]
    for nid, s in zip(ids, state):
        a, b = int(rng.integers(1, 6)), int(rng.integers(1, 9))
        if s == 3:
            a, b = (0, b) if rng.random() < 0.5 else (a, 0)
        on1, on2 = s != 2, s != 1
        if variant == 1:
            on2 = False
        if variant == 2:
            on1 = False
        B.related(nid, a, b, [0, 5, 20, 49, 50], on1=on1, on2=on2)
    return B.finish("disjoint_and_empty_nodes")


def _bow_unsorted(rng):
    """side-2 lists in shuffled index order holding duplicate descriptors: list order, not index order, breaks the tie (host entry points)"""
    B = _BowBuilder(rng)
    for nid in _node_ids(rng, int(rng.integers(3, 7))):
        a, b = int(rng.integers(1, 8)), int(rng.choice([4, 30, 70, 131]))
        d1 = rng.integers(0, 256, (a, 32), dtype=np.uint8)
        d2 = rng.integers(0, 256, (b, 32), dtype=np.uint8)
        for r in range(a):
            pos = rng.choice(b, min(b, int(rng.integers(2, 5))), replace=False)
            d2[pos] = _near(rng, d1[r], [int(rng.integers(0, 30))])[0]            # the same descriptor several times
        B.add(nid, d1, d2)
    return B.finish("unsorted_lists", shuffle2=True, ratio=float(rng.choice([1.5, 2.0, 1.0])))


def _bow_mixed(rng, n1=None, n2=None, n_nodes=None, **params):
    """features labelled with random nodes, side 2 mostly copies of side-1 features of the same node; random masks and parameters"""
    n1 = int(rng.integers(0, 600)) if n1 is None else n1
    n2 = int(rng.integers(0, 600)) if n2 is None else n2
    n_nodes = int(rng.choice([1, 7, 60, 300])) if n_nodes is None else n_nodes
    ids = _node_ids(rng, max(n_nodes, 1))[:n_nodes]
    lab1 = ids[rng.integers(0, n_nodes, n1)] if n_nodes else np.full(n1, -1, np.int64)
    lab1 = np.where(rng.random(n1) < 0.05, -1, lab1).astype(np.int64)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    k1, k2 = _bow_kps(rng, n1), _bow_kps(rng, n2)
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    lab2 = (ids[rng.integers(0, n_nodes, n2)] if n_nodes else np.full(n2, -1)).astype(np.int64)
    if n1 and n2:
        src = rng.integers(0, n1, n2)
        own = rng.random(n2) < 0.8
        d2 = np.where(own[:, None], flip_bits(rng, d1[src], rng.choice([0, 3, 10, 25, 49, 50, 51], n2)), d2)
        lab2 = np.where(own, lab1[src], lab2)
        k2["angle"] = np.where(own, (k1["angle"][src] + rng.choice([0.0, 0.0, 0.0, 90.0, 15.0], n2)) % np.float32(359.99), k2["angle"])
    fv1, fv2 = _featvec_from_labels(lab1), _featvec_from_labels(lab2)
    case = dict(kind="mixed", k1=k1, d1=d1, fv1=fv1, k2=k2, d2=d2, fv2=fv2,
                keep1=None if rng.random() < 0.3 else (rng.random(n1) < 0.85).astype(np.uint8),
                keep2=None if rng.random() < 0.3 else (rng.random(n2) < 0.85).astype(np.uint8),
                F12=None, size_ref=31.0, sigma_ref=1.0, score_threshold=float(rng.choice([50.0, 90.0, 30.5])), ratio=float(rng.choice([0.6, 0.8, 0.9, 1.0])),
                check_rotation=int(rng.integers(0, 2)), host_only=False)
    if rng.random() < 0.3:
        case.update(F12=(rng.normal(0, 1, (3, 3)) * np.array([[1e-5, 1e-5, 1e-2], [1e-5, 1e-5, 1e-2], [1e-2, 1e-2, 1.0]])).astype(np.float32),
                    sigma_ref=float(rng.choice([1.0, 400.0, 1e5])))
    case.update(params)
    return case


def bow_edge_cases(seed):
    """Cases for hs_search_by_bow / _ex / _legacy, each a dict tagged with `kind` (one of BOW_KINDS; a kind may come more than once per seed) that
    carries its own score_threshold, ratio, check_rotation, keep1, keep2, F12, size_ref, sigma_ref.  host_only marks feature vectors a DBoW2
    transform cannot produce (unsorted lists): they are for the entry points that take feature vectors from the host."""
    rng = np.random.default_rng(seed)
    yield _bow_ties(rng)
    yield _bow_list_sizes(rng)
    yield _bow_single(rng)
    yield _bow_thresholds(rng)
    yield _bow_thresholds(rng, thr=BOW_THRESHOLDS[seed % len(BOW_THRESHOLDS)], ratio=BOW_RATIOS[seed % len(BOW_RATIOS)])
    yield _bow_rotation(rng)
    yield _bow_rotation(rng, "three_maxima", THREE_MAXIMA_COUNTS[seed % len(THREE_MAXIMA_COUNTS)])
    yield _bow_rotation(rng, "three_maxima", THREE_MAXIMA_COUNTS[int(rng.integers(0, len(THREE_MAXIMA_COUNTS)))])
    for variant in ("bound", "den0", "nonfinite"):
        yield _bow_epipolar(rng, variant)
    yield _bow_competition(rng)
    yield _bow_disjoint(rng, 0)
    yield _bow_disjoint(rng, 1 + seed % 2)
    yield _bow_unsorted(rng)
    yield _bow_mixed(rng)


def bow_size_cases(seed):
    """n1 / n2 of 0, 1, 65 535 and above 65 535 (the host entry points take int32 indices), no node on one side, one node holding everything,
    as many nodes as features"""
    rng = np.random.default_rng(seed)
    yield _bow_mixed(rng, 0, 5, 2)
    yield _bow_mixed(rng, 5, 0, 2)
    yield _bow_mixed(rng, 1, 1, 1, keep1=None, keep2=None)
    yield _bow_disjoint(rng, 1)
    yield _bow_mixed(rng, 2000, 2000, 1)                                          # one node holds everything
    yield _bow_mixed(rng, 1500, 1500, 1500)                                       # about as many nodes as features
    yield _bow_mixed(rng, 65535, 65535, 600, F12=None, score_threshold=50.0, ratio=0.9, check_rotation=1)
    yield _bow_mixed(rng, 65600, 70000, 700, F12=None, score_threshold=50.0, ratio=0.9, check_rotation=0)


# ---- vocabulary trees
def flat_tree(rng, levels, children_of, orig_id=False, dup=0.0, zero_weight=0.0):
    """A flat forward-linked vocabulary tree in breadth-first order as dict(levels, n_nodes, child_begin, child_count, desc, word_id, weight,
    orig_id).  children_of(index, level, siblings) -> number of children (0 = leaf; forced to 0 at `levels`).  A child's descriptor is its
    parent's with bits flipped; `dup` = share of children that copy their left sibling (equal distances), `zero_weight` = share of words with
    a weight that is not positive."""
    cb, cc, level, desc = [0], [0], [0], [rng.integers(0, 256, 32, dtype=np.uint8)]
    i = 0
    while i < len(cb):
        c = 0 if level[i] >= levels else int(children_of(i, level[i], len(cb)))
        if i == 0:
            c = max(c, 1)
        cb[i], cc[i] = (len(cb) if c else 0), c
        if c:
            kids = flip_bits(rng, np.repeat(desc[i][None], c, 0), rng.integers(8, 120, c))
            for j in range(1, c):
                if rng.random() < dup:
                    kids[j] = kids[j - 1]
            for j in range(c):
                cb.append(0); cc.append(0); level.append(level[i] + 1); desc.append(kids[j])
        i += 1
    n = len(cb)
    cc_a = np.array(cc, np.int32)
    leaves = np.nonzero(cc_a == 0)[0]
    word = np.full(n, -1, np.int32); word[leaves] = np.arange(len(leaves))
    weight = np.zeros(n, np.float32); weight[leaves] = rng.uniform(0.5, 9.0, len(leaves))
    z = leaves[rng.random(len(leaves)) < zero_weight]
    weight[z] = rng.choice(np.array([0.0, -0.0, -1.5, 1e-42], np.float32), len(z))        # 1e-42 (subnormal) is > 0 and stays in the feature vector
    oid = None
    if orig_id:
        oid = (rng.permutation(n) * 5 + 11).astype(np.int32)
    return dict(levels=levels, n_nodes=n, child_begin=np.array(cb, np.int32), child_count=cc_a, desc=np.ascontiguousarray(np.stack(desc), np.uint8),
                word_id=word, weight=weight, orig_id=oid, level=np.array(level, np.int32))


def tree_struct(cls, tree):
    """the ctypes hs_vocab_tree / hso_vocab_tree of a flat_tree dict (the dict keeps the arrays alive)"""
    return cls(tree["n_nodes"], tree["levels"], tree["child_begin"].ctypes.data, tree["child_count"].ctypes.data, tree["desc"].ctypes.data,
               tree["word_id"].ctypes.data, tree["weight"].ctypes.data, None if tree["orig_id"] is None else tree["orig_id"].ctypes.data)


def tree_descriptors(rng, tree, n_random=60):
    """descriptors aimed at a tree: exact node descriptors, descriptors equidistant to two siblings, at distance 256 from a child, random"""
    nd, cb, cc = tree["desc"], tree["child_begin"], tree["child_count"]
    n = tree["n_nodes"]
    out = [rng.integers(0, 256, (n_random, 32), dtype=np.uint8), nd[rng.integers(0, n, 40)], np.bitwise_not(nd[rng.integers(1, n, 10)]),
           flip_bits(rng, nd[rng.integers(1, n, 40)], rng.integers(0, 30, 40))]
    parents = np.nonzero(cc >= 2)[0]
    for p in rng.choice(parents, min(len(parents), 30), replace=False) if len(parents) else []:
        j = cb[p] + int(rng.integers(0, cc[p] - 1))
        diff = np.unpackbits(nd[j] ^ nd[j + 1], bitorder="little")
        bits = np.nonzero(diff)[0]
        half = rng.permutation(bits)[:len(bits) // 2]                              # even difference: exactly equidistant to both siblings
        m = np.zeros(256, np.uint8); m[half] = 1
        out.append((nd[j] ^ np.packbits(m, bitorder="little"))[None])
    return np.ascontiguousarray(np.concatenate(out), np.uint8)


def vocab_edge_trees(seed):
    """Flat trees that are not complete uniform k-ary trees, each with descriptors aimed at it and the levelsup values to try.  `upload_refused`:
    levelsup values for which the feature-vector level has more than 8192 nodes (hs_vocab_upload must answer HS_ERR_INVALID)."""
    rng = np.random.default_rng(seed)
    specs = [
        ("shallow_leaf", 3, lambda i, lv, m: 0 if (lv == 1 and i % 3 == 1) or (lv == 2 and i % 4 == 0) else int(rng.integers(2, 5)), {}),
        ("ragged", 4, lambda i, lv, m: int(rng.choice([1, 2, 5, 17])) if lv < 2 or rng.random() < 0.7 else 0, {}),
        ("renumbered", 3, lambda i, lv, m: int(rng.integers(2, 7)), dict(orig_id=True)),
        ("ties_zero_weight", 3, lambda i, lv, m: int(rng.integers(2, 6)), dict(dup=0.4, zero_weight=0.4)),
        ("renumbered_shallow_ties", 4, lambda i, lv, m: 0 if lv >= 1 and rng.random() < 0.25 else int(rng.integers(1, 5)), dict(orig_id=True, dup=0.3, zero_weight=0.2)),
    ]
    for name, L, fn, kw in specs:
        t = flat_tree(rng, L, fn, **kw)
        yield dict(name=name, tree=t, desc=tree_descriptors(rng, t), levelsups=(0, 1, 2, L, L + 2), upload_refused=())
    t = flat_tree(rng, 2, lambda i, lv, m: 64 if lv == 0 else 128)                 # 8192 nodes at level 2
    yield dict(name="wide8192", tree=t, desc=tree_descriptors(rng, t, 300), levelsups=(0, 1, 2), upload_refused=())
    t = flat_tree(rng, 2, lambda i, lv, m: 64 if lv == 0 else (129 if i == 7 else 128))     # 8193
    yield dict(name="wide8193", tree=t, desc=tree_descriptors(rng, t, 300), levelsups=(0, 1), upload_refused=(0,))


# ---- brute-force 2-NN
KNN2_SIZES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1000)


def knn2_edge_cases(seed):
    """(kind, q, t): every size of KNN2_SIZES as nq and as nt; train sets all identical, all at one distance from the query, the query's complement
    (distance 256), duplicates of the best in different lanes and in the same lane (j and j + 64)"""
    rng = np.random.default_rng(seed)
    R = lambda n: rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for nq, nt in zip(rng.permutation(KNN2_SIZES), rng.permutation(KNN2_SIZES)):
        q, t = R(int(nq)), R(int(nt))
        if nq and nt:
            hit = rng.integers(0, nq, min(nt, 40))
            t[rng.choice(nt, len(hit), replace=False)] = flip_bits(rng, q[hit], rng.integers(0, 20, len(hit)))
        yield dict(kind="sizes", q=q, t=t)
    nt = int(rng.choice([2, 64, 65, 129, 200]))
    yield dict(kind="identical", q=R(5), t=np.repeat(R(1), nt, 0))
    q = R(int(rng.choice([1, 4, 7])))
    yield dict(kind="one_distance", q=q, t=_near(rng, q[0], np.full(nt, int(rng.integers(0, 200)))))
    yield dict(kind="complement", q=q, t=np.repeat(np.bitwise_not(q[:1]), nt, 0))
    q, t = R(6), R(200)
    j = int(rng.integers(0, 130))
    t[[j, j + 64]] = q[0]                                                         # the same lane
    t[[j + 1, j + 6]] = _near(rng, q[1], [3])[0]                                  # different lanes
    t[[199, 0]] = q[2] if j > 1 else t[[199, 0]]
    t[[j + 2, j + 66, j + 3]] = _near(rng, q[3], [9, 9, 8])                       # unique best, tied seconds
    yield dict(kind="duplicates", q=q, t=t)


# ---- frame records
def record_edge_sets(seed, pool=None):
    """Packed frame records for hs_records_bow_match_device / hs_records_knn2_device: dict(world, rank, cap, stride, buf (uint8 [world * stride]),
    frames = [(kps, desc)] as the device sees them: cut to the header count clamped to [0, cap]).  Peers hold flipped copies of the rank's
    descriptors; `pool` = descriptors to draw from (vocabulary node descriptors, so that the features spread over a tree's words).
    The set with cap = 65 535 is tagged big=True."""
    from hyslam_amd.distributed import pack_record, record_bytes
    rng = np.random.default_rng(seed)
    sets = [  # world, rank, cap, extra stride, counts, header overrides {record: raw header}
        (1, 0, 3, 0, [2], {}),
        (2, 1, 1, 0, [1, 1], {}),
        (2, 0, 3, 16, [3, 0], {}),
        (2, 1, 64, 0, [5, 0], {}),                                                # the rank's own record is short, the peer's empty
        (5, 2, 64, 0, [64, 1, 40, 64, 64], {0: 64 + 1000, 3: -5}),
        (5, 4, 301, 48, [301, 0, 1, 150, 299], {}),
        (5, 0, 300, 32, [300, 300, 17, 300, 64], {1: 300 + 1000, 0: 300 + 1000}),
        (2, 0, 65535, 0, [65535, 3000], {}),
    ]
    for world, rank, cap, extra, counts, hdr in sets:
        stride = record_bytes(cap) + extra
        base_n = max(counts[rank], 1)
        src = rng.integers(0, 256, (base_n, 32), dtype=np.uint8) if pool is None else \
            flip_bits(rng, pool[rng.integers(0, len(pool), base_n)], rng.integers(0, 12, base_n))
        buf = np.zeros(world * stride, np.uint8)
        frames = []
        for r in range(world):
            n = counts[r]
            k = _bow_kps(rng, n)
            if r == rank:
                d = src[:n].copy()
            else:
                pick = rng.integers(0, base_n, n)
                d = flip_bits(rng, src[pick], rng.choice([0, 2, 9, 30, 49, 50, 60], n))
                k["angle"] = np.float32(rng.choice([0.0, 15.0, 30.0, 200.0], n))
            rec = pack_record(k, d, cap)
            raw = hdr.get(r, n)
            rec[:4] = np.frombuffer(np.int32(raw).tobytes(), np.uint8)
            buf[r * stride:r * stride + len(rec)] = rec
            seen = min(max(raw, 0), cap)
            frames.append((k[:seen].copy(), d[:seen].copy()))
        yield dict(world=world, rank=rank, cap=cap, stride=stride, buf=buf, frames=frames, big=cap > 2000)
