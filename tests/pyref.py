"""Independent numpy restatement of the primitives the oracle implements in C++ (test infrastructure).

Written from the specification text, vectorised over whole images, so that it
shares no code structure with oracle/hs_oracle.cpp: an indexing or rounding slip in either shows up as a
disagreement.  Slow; used on small inputs only.
"""
import numpy as np

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
        (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
TAPS = np.array([18, 34, 49, 55, 49, 34, 18], np.int64)
UMAX = [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]


def cv_round(v):
    return np.rint(v).astype(np.int64)          # round half to even, like cvtss2si


def resize_linear(src, dw, dh):
    sh, sw = src.shape
    S = src.astype(np.int64)

    def table(dn, sn, clamp_weights):
        scale = 1.0 / (np.float64(dn) / np.float64(sn))
        d = np.arange(dn, dtype=np.float64)
        f = ((d + 0.5) * scale - 0.5).astype(np.float32)
        s = np.floor(f).astype(np.int64)
        f = (f - s.astype(np.float32)).astype(np.float32)
        if clamp_weights:
            low = s < 0
            f[low] = 0
            s[low] = 0
            high = s >= sn - 1
            f[high] = 0
            s[high] = sn - 1
        a0 = np.clip(cv_round((np.float32(1.0) - f) * np.float32(2048)), -32768, 32767)
        a1 = np.clip(cv_round(f * np.float32(2048)), -32768, 32767)
        return s, a0, a1

    sx, a0, a1 = table(dw, sw, True)
    sy, b0, b1 = table(dh, sh, False)
    sx1 = np.minimum(sx + 1, sw - 1)
    Hrows = S[:, sx] * a0[None, :] + S[:, sx1] * a1[None, :]            # (sh, dw)
    r0 = np.clip(sy, 0, sh - 1)
    r1 = np.clip(sy + 1, 0, sh - 1)
    H0, H1 = Hrows[r0], Hrows[r1]
    out = (((b0[:, None] * (H0 >> 4)) >> 16) + ((b1[:, None] * (H1 >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def preprocess(src, rgb, fscale):
    """ImageProcessing::PreProcessImg (src/main/ImageProcessing.cpp:118-138) from the text of OpenCV 3.4's resize / cvtColor: vectorised over the frame
    (the oracle walks pixels).  src (h, w) or (h, w, cn) uint8."""
    if src.ndim == 2:
        src = src[:, :, None]
    sh, sw, cn = src.shape
    inv = np.float64(np.float32(fscale))
    dw, dh = int(np.rint(sw * inv)), int(np.rint(sh * inv))
    scale = 1.0 / inv
    S = src.astype(np.int64)
    if (dw, dh) == (sw, sh):
        col = S
    elif abs(scale - np.rint(scale)) < np.finfo(np.float64).eps and int(np.rint(scale)) == 2:
        # INTER_LINEAR at exactly 1/2 is INTER_AREA's fast path: rounded 2x2 means for the full blocks, float means of what exists for trailing partial ones
        pad = np.zeros((2 * dh + 2, 2 * dw + 2, cn), np.int64)
        msk = np.zeros((2 * dh + 2, 2 * dw + 2, 1), np.int64)
        hh, ww = min(sh, 2 * dh), min(sw, 2 * dw)
        pad[:hh, :ww] = S[:hh, :ww]
        msk[:hh, :ww] = 1
        blk = lambda a: a[0:2 * dh:2, 0:2 * dw:2] + a[0:2 * dh:2, 1:2 * dw:2] + a[1:2 * dh:2, 0:2 * dw:2] + a[1:2 * dh:2, 1:2 * dw:2]
        ssum, cnt = blk(pad), blk(msk)
        full = (np.arange(dw)[None, :, None] < sw // 2) & (2 * np.arange(dh)[:, None, None] + 1 < sh)
        fast = (ssum + 2) >> 2
        with np.errstate(divide="ignore", invalid="ignore"):
            slow = np.where(cnt > 0, np.rint(ssum.astype(np.float32) / np.maximum(cnt, 1).astype(np.float32)), 0).astype(np.int64)
        col = np.where(full, fast, np.clip(slow, 0, 255))
    else:
        def table(dn, sn, clamp_weights):
            d = np.arange(dn, dtype=np.float64)
            f = ((d + 0.5) * scale - 0.5).astype(np.float32)
            s_ = np.floor(f).astype(np.int64)
            f = (f - s_.astype(np.float32)).astype(np.float32)
            if clamp_weights:
                low = s_ < 0
                f[low] = 0; s_[low] = 0
                high = s_ >= sn - 1
                f[high] = 0; s_[high] = sn - 1
            a0 = np.clip(cv_round((np.float32(1.0) - f) * np.float32(2048)), -32768, 32767)
            a1 = np.clip(cv_round(f * np.float32(2048)), -32768, 32767)
            return s_, a0, a1
        sx, a0, a1 = table(dw, sw, True)
        sy, b0, b1 = table(dh, sh, False)
        sx1 = np.minimum(sx + 1, sw - 1)
        H = S[:, sx] * a0[None, :, None] + S[:, sx1] * a1[None, :, None]
        H0, H1 = H[np.clip(sy, 0, sh - 1)], H[np.clip(sy + 1, 0, sh - 1)]
        col = (((b0[:, None, None] * (H0 >> 4)) >> 16) + ((b1[:, None, None] * (H1 >> 4)) >> 16) + 2) >> 2
    if cn == 1:
        return col[:, :, 0].astype(np.uint8)
    r, g, b = (col[:, :, 0], col[:, :, 1], col[:, :, 2]) if rgb else (col[:, :, 2], col[:, :, 1], col[:, :, 0])
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def fast_scores(img, t=20):
    """Score map (0 = not a corner) over the whole view; only [3,h-3) x [3,w-3) can be non-zero."""
    h, w = img.shape
    I = img.astype(np.int64)
    c = I[3:h - 3, 3:w - 3]
    ring = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING])      # (16, H, W)
    d = c[None] - ring
    dark = d > t                 # ring < v - t
    bright = d < -t              # ring > v + t

    def arc9(m):
        mm = np.concatenate([m, m[:8]], 0)
        ok = np.zeros(m.shape[1:], bool)
        for k in range(16):
            ok |= mm[k:k + 9].all(0)
        return ok

    corner = arc9(dark) | arc9(bright)
    dd = np.concatenate([d, d[:8]], 0)
    amin = np.max(np.stack([dd[k:k + 9].min(0) for k in range(16)]), 0)
    amax = np.max(np.stack([(-dd[k:k + 9]).min(0) for k in range(16)]), 0)
    score = np.maximum(np.maximum(amin, amax), t) - 1
    out = np.zeros((h, w), np.int64)
    out[3:h - 3, 3:w - 3] = np.where(corner, score, 0)
    return out


def fast(img, t=20, nonmax=True):
    """-> rows (x, y, score) in scan order."""
    h, w = img.shape
    if h < 7 or w < 7:
        return np.zeros((0, 3), np.int64)
    s = fast_scores(img, t)
    keep = s > 0
    if nonmax:
        p = np.pad(s, 1)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx or dy:
                    keep &= s > p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    ys, xs = np.nonzero(keep)
    return np.stack([xs, ys, s[ys, xs]], 1)


def gaussian_blur7(img, taps=TAPS):
    taps = np.asarray(taps, np.int64)
    p = np.pad(img.astype(np.int64), 3, mode="reflect")        # numpy 'reflect' == BORDER_REFLECT_101
    h, w = img.shape
    hor = np.zeros((h + 6, w), np.int64)
    for k in range(7):
        hor = np.minimum(hor + np.minimum(taps[k] * p[:, k:k + w], 0xFFFF), 0xFFFF)
    ver = np.zeros((h, w), np.int64)
    for k in range(7):
        ver = np.minimum(ver + taps[k] * hor[k:k + h], 0xFFFFFFFF)
    return np.minimum((ver + 0x8000) >> 16, 255).astype(np.uint8)


def fast_atan2(y, x):
    f = np.float32
    k = f(180.0 / np.pi)
    p1, p3, p5, p7 = (f(0.9997878412794807) * k, f(-0.3258083974640975) * k, f(0.1555786518463281) * k, f(-0.04432655554792128) * k)
    x, y = f(x), f(y)
    ax, ay = f(abs(x)), f(abs(y))
    eps = f(2.2204460492503131e-16)
    if ax >= ay:
        c = f(ay / f(ax + eps))
        c2 = f(c * c)
        a = f(f(f(f(f(f(f(p7 * c2) + p5) * c2) + p3) * c2) + p1) * c)
    else:
        c = f(ax / f(ay + eps))
        c2 = f(c * c)
        a = f(f(90.0) - f(f(f(f(f(f(f(p7 * c2) + p5) * c2) + p3) * c2) + p1) * c))
    if x < 0:
        a = f(f(180.0) - a)
    if y < 0:
        a = f(f(360.0) - a)
    return a


def ic_angle(blurred, x, y):
    cx, cy = int(np.rint(np.float32(x))), int(np.rint(np.float32(y)))
    m10 = m01 = 0
    for v in range(-15, 16):
        d = UMAX[abs(v)]
        row = blurred[cy + v, cx - d:cx + d + 1].astype(np.int64)
        u = np.arange(-d, d + 1)
        m10 += int((u * row).sum())
        m01 += v * int(row.sum())
    return fast_atan2(np.float32(m01), np.float32(m10))


def orb_descriptor(blurred, x, y, angle, pattern):
    f = np.float32
    cx, cy = int(np.rint(f(x))), int(np.rint(f(y)))
    theta = f(f(angle) * f(np.pi / f(180.0)))
    a, b = f(np.cos(np.float64(theta))), f(np.sin(np.float64(theta)))
    pat = np.asarray(pattern, np.int64).reshape(512, 2).astype(np.float32)
    px, py = pat[:, 0], pat[:, 1]
    dy = np.rint((px * b).astype(f) + (py * a).astype(f)).astype(np.int64)
    dx = np.rint((px * a).astype(f) - (py * b).astype(f)).astype(np.int64)
    vals = blurred[cy + dy, cx + dx].astype(np.int64).reshape(256, 2)
    bits = (vals[:, 0] < vals[:, 1]).astype(np.uint8)
    return np.packbits(bits.reshape(32, 8), axis=1, bitorder="little").ravel()


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def distribute_octtree(cands, min_x, max_x, min_y, max_y, n_target):
    """SURVEY.md §8a.1 R1 step 3, with tie-break D1 (creation order stands in for the node address).
    cands: rows (x, y, response).  Returns indices of the kept candidates in final list order."""
    import math
    W, Hh = max_x - min_x, max_y - min_y
    n_ini = int(math.floor(np.float32(W) / np.float32(Hh) + np.float32(0.5)))      # round() of a positive float
    if n_ini < 1:
        return []
    hx = np.float32(W) / np.float32(n_ini)
    seq = [0]

    def node(x0, x1, y0, y1, pts):
        seq[0] += 1
        return dict(x0=x0, x1=x1, y0=y0, y1=y1, pts=pts, seq=seq[0])

    def split(nd):
        mx = nd["x0"] + int(math.ceil((nd["x1"] - nd["x0"]) / 2.0))
        my = nd["y0"] + int(math.ceil((nd["y1"] - nd["y0"]) / 2.0))
        quads = [[], [], [], []]
        for i in nd["pts"]:
            quads[(0 if cands[i][0] < mx else 1) + (0 if cands[i][1] < my else 2)].append(i)
        b = [(nd["x0"], mx, nd["y0"], my), (mx, nd["x1"], nd["y0"], my), (nd["x0"], mx, my, nd["y1"]), (mx, nd["x1"], my, nd["y1"])]
        return [node(*b[q], quads[q]) for q in range(4) if quads[q]]

    roots = [node(int(hx * np.float32(i)), int(hx * np.float32(i + 1)), 0, Hh, []) for i in range(n_ini)]
    for i, c in enumerate(cands):
        roots[int(np.float32(c[0]) / hx)]["pts"].append(i)
    nodes = [r for r in roots if r["pts"]]                  # front ... back
    fresh = []
    done = False
    while not done:
        prev = len(nodes)
        new_front, keep, fresh = [], [], []
        for nd in nodes:
            if len(nd["pts"]) == 1:
                keep.append(nd)
                continue
            ch = split(nd)
            new_front = ch[::-1] + new_front               # each child is pushed to the front in turn
            fresh += [c for c in ch if len(c["pts"]) > 1]
        nodes = new_front + keep
        if len(nodes) >= n_target or len(nodes) == prev:
            done = True
        elif len(nodes) + 3 * len(fresh) > n_target:
            while not done:
                prev = len(nodes)
                order = sorted(fresh, key=lambda n: (len(n["pts"]), n["seq"]))
                fresh = []
                for nd in reversed(order):
                    ch = split(nd)
                    idx = next(k for k, m in enumerate(nodes) if m is nd)
                    nodes.pop(idx)
                    nodes = ch[::-1] + nodes
                    fresh += [c for c in ch if len(c["pts"]) > 1]
                    if len(nodes) >= n_target:
                        break
                if len(nodes) >= n_target or len(nodes) == prev:
                    done = True
    out = []
    for nd in nodes:
        best = nd["pts"][0]
        for i in nd["pts"][1:]:
            if cands[i][2] > cands[best][2]:
                best = i
        out.append(best)
    return out


_POPCOUNT8 = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int64)


def stereo_match(kpsL, descL, kpsR, descR, fx, mbf, n_rows, th_high, th_low, size_ref):
    """Stereomatcher::computeStereoMatches (src/features/Stereomatcher.cpp:36-156) with deviation D2.

    Built without the reference's row table: each left keypoint takes a mask over ALL right keypoints (row band, octave, disparity
    window), and its best match is the first index of the smallest distance among them.  Every quantity is fp32 as in the reference.
    -> (uRight, depth, best_idx, best_dist); best_idx / best_dist are -1 where uRight is -1 before the median cut."""
    f = np.float32
    nL, nR = len(kpsL), len(kpsR)
    uRight = np.full(nL, -1, f)
    depth = np.full(nL, -1, f)
    best_idx = np.full(nL, -1, np.int32)
    best_dist = np.full(nL, -1, np.int32)
    th_high, th_low, fx, mbf, size_ref = f(th_high), f(th_low), f(fx), f(mbf), f(size_ref)
    accept = f(f(th_high + th_low) / f(2))
    mb = f(mbf / fx)
    max_d = f(mbf / mb)                                     # minZ = mb; minD = 0
    yR = np.asarray(kpsR["y"], f)
    xR = np.asarray(kpsR["x"], f)
    octR = np.asarray(kpsR["octave"], np.int64)
    band = (f(2) * np.asarray(kpsR["size"], f) / size_ref).astype(f)
    top = np.ceil((yR + band).astype(f)).astype(np.int64)    # a right keypoint covers rows floor(y - r) .. ceil(y + r)
    bottom = np.floor((yR - band).astype(f)).astype(np.int64)
    dR = np.asarray(descR, np.uint8).reshape(nR, 32)
    dL = np.asarray(descL, np.uint8).reshape(nL, 32)
    accepted = []                                           # (distance, iL)
    for iL in range(nL):
        vL, uL, levelL = f(kpsL["y"][iL]), f(kpsL["x"][iL]), int(kpsL["octave"][iL])
        if not vL >= 0:
            continue
        row = int(np.floor(vL))
        if row >= n_rows:                                   # also every row when n_rows <= 0 (D2)
            continue
        in_row = (bottom <= row) & (row <= top)             # rows outside [0, n_rows) were never listed, but `row` is inside
        if not in_row.any():
            continue
        min_u, max_u = f(uL - max_d), f(uL - f(0))
        if max_u < 0:
            continue
        cand = np.nonzero(in_row & (octR >= levelL - 1) & (octR <= levelL + 1) & (xR >= min_u) & (xR <= max_u))[0]
        best, best_r = th_high, 0                           # the reference's initial values, kept when nothing beats TH_HIGH
        if len(cand):
            dist = _POPCOUNT8[np.bitwise_xor(dR[cand], dL[iL])].sum(1)
            k = int(np.argmin(dist))                        # the first of equal minima: the lowest iR
            if f(dist[k]) < th_high:
                best, best_r = f(dist[k]), int(cand[k])
        if not best < accept:
            continue
        u_r = xR[best_r] if nR else f(0)
        disparity = f(uL - u_r)
        if not (disparity >= 0 and disparity < max_d):
            continue
        if disparity <= 0:
            disparity = f(0.01)
            u_r = f(np.float64(uL) - 0.01)
        uRight[iL] = u_r
        depth[iL] = f(mbf / disparity)
        best_idx[iL] = best_r
        best_dist[iL] = int(best)
        accepted.append((best, iL))
    if accepted:                                            # D2: no match, no cut
        accepted.sort()
        th_dist = f(f(1.5) * f(1.4)) * accepted[len(accepted) // 2][0]
        for d, iL in accepted:
            if not d < th_dist:
                uRight[iL] = -1
                depth[iL] = -1
    return uRight, depth, best_idx, best_dist


# ---------------------------------------------------------------- grid-area queries and the loop-closing matchers
# Frame.cc:137-153,416-469 (grid, GetFeaturesInAreaNEW), KeyFrame.cc:258-279,329-374 (landMarkSizePixels, GetFeaturesInArea, IsInImage),
# Camera.cpp:116-153 (Project), FeatureMatcher.cc:628-934 (SearchByProjection(pKF, Scw, ...), SearchBySim3).
# Float expressions are evaluated one float32 operation at a time; cv::Mat products (gemm, norm, dot) accumulate float inputs in double, left to
# right, and round once.  Python floats are the doubles.
GRID_COLS, GRID_ROWS = 64, 48
INT_MIN = -(1 << 31)
_f = np.float32


def cvt_i32(v):
    """(int) of an integral float as hySLAM's x86-64 build converts it (cvttss2si): NaN or a value outside the int range gives INT_MIN."""
    v = np.asarray(v, np.float64)
    ok = (v >= -2147483648.0) & (v < 2147483648.0)
    return np.where(ok, np.where(ok, v, 0.0), float(INT_MIN)).astype(np.int64)


def _round_away(a):
    """std::round on float32: half away from zero (exact in double for every float)"""
    a = np.asarray(a, np.float64)
    return np.sign(a) * np.floor(np.abs(a) + 0.5)


def _grid_inv(bounds):
    minx, maxx, miny, maxy = (_f(b) for b in bounds)
    with np.errstate(all="ignore"):
        return minx, miny, _f(_f(GRID_COLS) / _f(maxx - minx)), _f(_f(GRID_ROWS) / _f(maxy - miny))


def frame_grid(kps, bounds):
    """Frame::PosInGrid of every keypoint -> (n, 2) int64, -1 outside the 64 x 48 grid"""
    minx, miny, invW, invH = _grid_inv(bounds)
    with np.errstate(all="ignore"):
        px = cvt_i32(_round_away(((kps["x"].astype(_f) - minx).astype(_f) * invW).astype(_f)))
        py = cvt_i32(_round_away(((kps["y"].astype(_f) - miny).astype(_f) * invH).astype(_f)))
    ok = (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)
    return np.stack([np.where(ok, px, -1), np.where(ok, py, -1)], 1)


class AreaGrid:
    """mGrid[ix][iy] of a frame: cell lists in keypoint index order (AssignFeaturesToGrid pushes in index order)"""

    def __init__(self, kps, bounds):
        self.kps, self.bounds = kps, bounds
        self.minx, self.miny, self.invW, self.invH = _grid_inv(bounds)
        self.cells = frame_grid(kps, bounds)
        inside = np.nonzero(self.cells[:, 0] >= 0)[0]
        key = self.cells[inside, 0] * GRID_ROWS + self.cells[inside, 1]           # column-major: the cells of one column are contiguous
        o = np.argsort(key, kind="stable")
        self.items = inside[o]
        self.start = np.searchsorted(key[o], np.arange(GRID_COLS * GRID_ROWS + 1))
        self.kx, self.ky = kps["x"].astype(_f), kps["y"].astype(_f)

    def features_in_area(self, x, y, r):
        """GetFeaturesInArea(x, y, r): cells walked ix outer, iy inner; |dx| < r and |dy| < r, strict.  -> indices in that order"""
        x, y, r = _f(x), _f(y), _f(r)
        empty = np.zeros(0, np.int64)
        with np.errstate(all="ignore"):
            x0 = max(0, int(cvt_i32(np.floor(_f(_f(_f(x - self.minx) - r) * self.invW)))))
            if x0 >= GRID_COLS:
                return empty
            x1 = min(GRID_COLS - 1, int(cvt_i32(np.ceil(_f(_f(_f(x - self.minx) + r) * self.invW)))))
            if x1 < 0:
                return empty
            y0 = max(0, int(cvt_i32(np.floor(_f(_f(_f(y - self.miny) - r) * self.invH)))))
            if y0 >= GRID_ROWS:
                return empty
            y1 = min(GRID_ROWS - 1, int(cvt_i32(np.ceil(_f(_f(_f(y - self.miny) + r) * self.invH)))))
            if y1 < 0:
                return empty
            spans = [self.items[self.start[ix * GRID_ROWS + y0]:self.start[ix * GRID_ROWS + y1 + 1]] for ix in range(x0, x1 + 1)]
            c = np.concatenate(spans) if spans else empty
            keep = (np.abs((self.kx[c] - x).astype(_f)) < r) & (np.abs((self.ky[c] - y).astype(_f)) < r)
        return c[keep]


def _gemm_row(a, b, c, alpha=1.0):
    """one row of a cv::Mat product alpha*A*B + C: float inputs, double accumulation, one rounding"""
    s = float(a[0]) * float(b[0]) + float(a[1]) * float(b[1]) + float(a[2]) * float(b[2])
    with np.errstate(all="ignore"):
        return _f(alpha * s + float(c))


def _norm(p):
    return _f(np.sqrt(float(p[0]) * float(p[0]) + float(p[1]) * float(p[1]) + float(p[2]) * float(p[2])))


def camera_project(fr, Pc):
    """Camera::Project(Pc, uv) -> (u, v, valid); valid: z > 0 and min <= u <= max, min <= v <= max (both bounds inclusive)"""
    z = _f(Pc[2])
    with np.errstate(all="ignore"):
        hx, hy, hz = _f(_f(Pc[0]) / z), _f(_f(Pc[1]) / z), _f(z / z)
        u = _f(float(fr["fx"]) * float(hx) + 0.0 * float(hy) + float(fr["cx"]) * float(hz))
        v = _f(0.0 * float(hx) + float(fr["fy"]) * float(hy) + float(fr["cy"]) * float(hz))
    minx, maxx, miny, maxy = (_f(b) for b in fr["bounds"])
    return u, v, bool(z > 0 and u >= minx and u <= maxx and v >= miny and v <= maxy)


def project_landmark(fr, P):
    """Frame / KeyFrame::ProjectLandMark with the frame's own pose: Pc = Rcw*P + tcw (one gemm), then Camera::Project"""
    R, t = np.asarray(fr["Rcw"], _f).reshape(3, 3), np.asarray(fr["tcw"], _f).reshape(3)
    return camera_project(fr, [_gemm_row(R[i], P, t[i]) for i in range(3)])


def landmark_size_px(fr, lm):
    """landMarkSizePixels: the associated keypoint's size, else the projected width of the landmark along world x (frame's own pose)"""
    if lm["assoc_kp"] >= 0:
        return _f(fr["kps"]["size"][lm["assoc_kp"]])
    p = lm["pos"].astype(_f)
    with np.errstate(all="ignore"):
        half = _f(_f(lm["size"]) / _f(2))
        ul = project_landmark(fr, [_f(p[0] - half), p[1], p[2]])[0]
        ur = project_landmark(fr, [_f(p[0] + half), p[1], p[2]])[0]
        return _f(ur - ul)


def _hamming_to(desc, idx, d):
    return np.unpackbits(desc[idx] ^ d[None, :], axis=1).sum(1)


def search_by_projection_sim3(fr, Scw, lms, th, th_low, kp_matched, grid=None):
    """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) -> (match_idx[L], kp_matched'[n], nmatches).  lms: min_dist / max_dist hold the
    invariance range, skip = bad or already found; kp_matched = vpMatched[idx] != NULL.  Landmarks are taken in order; a match takes its keypoint."""
    S = np.asarray(Scw, _f).reshape(4, 4)
    g = grid or AreaGrid(fr["kps"], fr["bounds"])
    size_ref = _f(fr.get("size_ref", 31.0))
    taken = np.asarray(kp_matched, np.uint8).copy()
    out = np.full(len(lms), -1, np.int32)
    with np.errstate(all="ignore"):
        scw = _f(np.sqrt(float(S[0, 0]) ** 2 + float(S[0, 1]) ** 2 + float(S[0, 2]) ** 2))       # sqrt(row0.dot(row0))
        inv = _f(1.0 / float(scw))                                                               # Mat / s: every element times (float)(1/s)
        Rcw = (S[:3, :3] * inv).astype(_f) + _f(0)
        tcw = (S[:3, 3] * inv).astype(_f) + _f(0)
        Ow = [_gemm_row(Rcw[:, i], tcw, 0.0, -1.0) for i in range(3)]                            # -Rcw.t()*tcw
    minx, maxx, miny, maxy = (_f(b) for b in fr["bounds"])
    fx, fy, cx, cy = _f(fr["fx"]), _f(fr["fy"]), _f(fr["cx"]), _f(fr["cy"])
    n = 0
    for i, lm in enumerate(lms):
        if lm["skip"]:
            continue
        p = lm["pos"].astype(_f)
        pc = [_gemm_row(Rcw[k], p, tcw[k]) for k in range(3)]
        if pc[2] < 0.0:
            continue
        with np.errstate(all="ignore"):
            invz = _f(_f(1) / pc[2])
            u = _f(_f(fx * _f(pc[0] * invz)) + cx)
            v = _f(_f(fy * _f(pc[1] * invz)) + cy)
        if not (u >= minx and u < maxx and v >= miny and v < maxy):                               # KeyFrame::IsInImage: upper bounds strict
            continue
        with np.errstate(all="ignore"):
            PO = [_f(p[k] - Ow[k]) for k in range(3)]
        dist = _norm(PO)
        if dist < lm["min_dist"] or dist > lm["max_dist"]:
            continue
        dot = float(PO[0]) * float(lm["normal"][0]) + float(PO[1]) * float(lm["normal"][1]) + float(PO[2]) * float(lm["normal"][2])
        if dot < 0.5 * float(dist):
            continue
        with np.errstate(all="ignore"):
            radius = _f(_f(_f(th) * landmark_size_px(fr, lm)) / size_ref)
        c = g.features_in_area(u, v, radius)
        c = c[taken[c] == 0]
        if len(c) == 0:
            continue
        d = _hamming_to(fr["desc"], c, lm["desc"])
        b = int(np.argmin(d))                                                                     # first minimum in candidate order
        if d[b] <= th_low:
            taken[c[b]] = 1
            out[i] = c[b]
            n += 1
    return out, taken, n


def search_by_sim3(fr1, lms1, fr2, lms2, s12, R12, t12, th, th_high, grids=None):
    """SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) -> (match12[n1], nFound).  lms1 / lms2: the landmark of each keypoint (skip = none,
    bad or already matched; assoc_kp = its keypoint in the OTHER keyframe).  Both directions, then the agreement check."""
    R12 = np.asarray(R12, _f).reshape(3, 3)
    t12 = np.asarray(t12, _f).reshape(3)
    g1, g2 = grids or (AreaGrid(fr1["kps"], fr1["bounds"]), AreaGrid(fr2["kps"], fr2["bounds"]))
    with np.errstate(all="ignore"):
        sR12 = (R12 * _f(float(s12))).astype(_f) + _f(0)                                         # s12*R12
        sR21 = (R12.T * _f(1.0 / float(_f(s12)))).astype(_f) + _f(0)                              # (1.0/s12)*R12.t()
        t21 = np.array([_gemm_row(sR21[k], t12, 0.0, -1.0) for k in range(3)], _f)                # -sR21*t12

    def direction(fsrc, lms, fdst, gdst, sR, tt):
        Rs, ts = np.asarray(fsrc["Rcw"], _f).reshape(3, 3), np.asarray(fsrc["tcw"], _f).reshape(3)
        size_ref = _f(fdst.get("size_ref", 31.0))
        out = np.full(len(lms), -1, np.int64)
        for i, lm in enumerate(lms):
            if lm["skip"]:
                continue
            p = lm["pos"].astype(_f)
            ps = [_gemm_row(Rs[k], p, ts[k]) for k in range(3)]
            pd = [_gemm_row(sR[k], ps, tt[k]) for k in range(3)]
            u, v, ok = camera_project(fdst, pd)
            if not ok:
                continue
            d3 = _norm(pd)
            if d3 < lm["min_dist"] or d3 > lm["max_dist"]:
                continue
            with np.errstate(all="ignore"):
                radius = _f(_f(_f(th) * landmark_size_px(fdst, lm)) / size_ref)
            c = gdst.features_in_area(u, v, radius)
            if len(c) == 0:
                continue
            d = _hamming_to(fdst["desc"], c, lm["desc"])
            b = int(np.argmin(d))
            if d[b] <= th_high:
                out[i] = c[b]
        return out

    m1 = direction(fr1, lms1, fr2, g2, sR21, t21)
    m2 = direction(fr2, lms2, fr1, g1, sR12, t12)
    match12 = np.full(len(lms1), -1, np.int32)
    for i1, i2 in enumerate(m1):
        if i2 >= 0 and m2[i2] == i1:
            match12[i1] = i2
    return match12, int((match12 >= 0).sum())
