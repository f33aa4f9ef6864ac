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
