"""Directed scenes for the extractor's composition (tests/test_extract_ref.py on the CPU, tests/test_gpu_extract_edges.py on the GPU).

A case is a dict: edge (what it is there for), img, the extractor settings (nfeatures, scale, nlevels, n_cells, fast_threshold, blur_taps) and
`witness`, a function of the REFERENCE's output (keypoints, descriptors, debug dict of ref_extract.extract) that returns [(label, bool)]: proof
that the edge occurred in this run.  A false witness fails the CPU test; nothing is skipped.  Frames are at most 640 x 480, most at most 320 x 240.

Cell geometry with N_CELLS = 16 (extent E along one axis; border 16 on either side, first cell at 16):
  209  11 cells of 17: the last view is clipped to exactly 7 (one detectable line, E - 20)
  225  12 cells of 17: along x the last cell is skipped by `iniX >= maxBorderX-6`; along y the last row is KEPT by `iniY >= maxBorderY-3` and its
       views are 6 tall, so FAST finds nothing and every one of its cells is retried
  241  13 cells of 17: along x the second-to-last view is clipped and the last skipped; along y the last row is kept with views 5 tall
  273  15 cells of 17: the last row (3 left) is skipped by the `-3` rule, the last column (3 left) by the `-6` rule
No skip ever loses a corner (a view below 7 finds nothing), so the skip rules show in the statistics (cells run, retried, view sizes), not in the
keypoints: the witnesses read them there.

With the default 30 px cells none of these is reachable within 640 x 480: the last cell falls short of its neighbours only by the rounding of
wCell = ceil(width / nCols), less than one pixel a cell, so a last view of 7 or a skipped cell needs about 24 cells of 30 px, an extent above 700.
A search with ref_extract.cell_grid over every level (8 levels, scale 1.2 / 1.25 / 1.4 / 1.7 / 2.0) of the frames 640 x H, 300 <= H <= 480, finds no
level with a skipped, a 7-pixel or a shorter last view along either axis, so there is no such case here; 30 px cells run in the plain cases.

Slowest case on the CPU reference: plain_640x480 (1000 features, 8 levels), 1.0 s measured (reference 0.8 s + oracle and comparisons); every other
case stays below 0.6 s.
"""
import functools

import numpy as np

import pyref
from hyslam_amd.synth import synth_image, synth_stereo_pair

GEOM = dict(nfeatures=400, scale=1.2, nlevels=3, n_cells=16, fast_threshold=20, blur_taps=None)     # the settings the 273 x 225 frames share (one batch)


def _case(edge, img, witness, **kw):
    c = dict(GEOM)
    c.update(kw)
    c.update(edge=edge, img=np.ascontiguousarray(img, np.uint8), witness=witness)
    return c


def settings_of(c):
    return dict(nfeatures=c["nfeatures"], scale=c["scale"], nlevels=c["nlevels"], n_cells=c["n_cells"], fast_threshold=c["fast_threshold"], blur_taps=c["blur_taps"])


def _pad(img, x, y, r=5, bg=60, v=255):
    """a flat square of side 2r+1 around (x, y) with one bright pixel in its middle: exactly one FAST corner, score v - bg - 1, at (x, y)"""
    h, w = img.shape
    img[max(y - r, 0):min(y + r + 1, h), max(x - r, 0):min(x + r + 1, w)] = bg
    img[y, x] = v


def _has(c, x, y):
    """a candidate at level pixel (x, y)?  (candidates are relative to the border of 16)"""
    return bool(len(c)) and bool(((c[:, 0] == x - 16) & (c[:, 1] == y - 16)).any())


def _edge_frame(seed, w, h):
    """structured content with isolated corners on the last detectable column (w - 20) and row (h - 20) and one beyond each"""
    img = synth_image(seed, w, h)
    pts = [(w - 20, 40), (w - 20, h // 2), (w - 20, h - 20), (40, h - 20), (w // 2, h - 20), (w - 19, 80), (90, h - 19), (19, 19), (19, h - 20), (w - 20, 19)]
    for x, y in pts:
        _pad(img, x, y)
    return img


def _geom_witness(w, h, expect):
    def wit(k, d, g):
        st, c = g["stats"][0], g["candidates"][0]
        n_cols, n_rows = st["grid"][:2]
        out = [("corner on the last detectable column", _has(c, w - 20, 40) and _has(c, w - 20, h // 2)),
               ("corner on the last detectable row", _has(c, 40, h - 20) and _has(c, w // 2, h - 20)),
               ("corner in the last detectable corner pixel", _has(c, w - 20, h - 20) and _has(c, 19, 19)),
               ("nothing one past the last column / row", not _has(c, w - 19, 80) and not _has(c, 90, h - 19) and (c[:, 0] <= w - 36).all() and (c[:, 1] <= h - 36).all())]
        for label, f in expect.items():
            out.append((label, bool(f(st, n_cols, n_rows))))
        return out
    return wit


def _periodic(w=273, h=225, period=9, bg=40, v=255):
    """exactly periodic, no noise: node (9a, 9b) carries a horizontal pair of bright pixels, a single one or a vertical pair, by (b + 1) % 3.
    Every bright pixel has all 16 ring pixels darker by the same amount: one score everywhere.  A pair inside a cell is suppressed as a whole (strict
    maximum over 8 neighbours); a pair cut by a cell seam (x = 171 | 172, y = 171 | 172 with cells of 17 from 19) survives on both sides."""
    img = np.full((h, w), bg, np.uint8)
    for b in range(h // period + 1):
        for a in range(w // period + 1):
            x, y, t = period * a, period * b, (b + 1) % 3
            for dx, dy in ((0, 0),) + (((1, 0),) if t == 0 else ((0, 1),) if t == 2 else ()):
                if x + dx < w and y + dy < h:
                    img[y + dy, x + dx] = v
    return img


def _cell_of_pixels(st, xs, ys):
    _, _, wc, hc = st["grid"]
    return (xs - 19) // wc, (ys - 19) // hc


def _seam_witness(k, d, g):
    st, c = g["stats"][0], g["candidates"][0]
    xs, ys = c[:, 0].astype(np.int64) + 16, c[:, 1].astype(np.int64) + 16
    cell = np.array(st["cell_of"])
    key = {(int(x), int(y)): tuple(cl) for x, y, cl in zip(xs, ys, cell)}
    across = 0
    for (x, y), cl in key.items():
        for dx, dy in ((1, 0), (0, 1), (1, 1), (1, -1)):
            o = key.get((x + dx, y + dy))
            if o is not None and o != cl:
                across += 1
    s = pyref.fast_scores(g["pyramid"][0], 20)
    cand = np.zeros(s.shape, bool)
    cand[ys, xs] = True
    h, w = s.shape
    inside = 0
    for dx, dy in ((1, 0), (0, 1)):
        a, b = s[19:h - 20 - dy, 19:w - 20 - dx], s[19 + dy:h - 20, 19 + dx:w - 20]
        yy, xx = np.nonzero((a > 0) & (a == b))
        yy, xx = yy + 19, xx + 19
        ja, ia = _cell_of_pixels(st, xx, yy)
        jb, ib = _cell_of_pixels(st, xx + dx, yy + dy)
        same = (ja == jb) & (ia == ib)
        inside += int((same & ~cand[yy, xx] & ~cand[yy + dy, xx + dx]).sum())
    return [("8-adjacent candidates kept on either side of a cell seam", across >= 1),
            ("equal-score neighbours inside a cell, both suppressed", inside >= 1),
            ("one score on level 0", len(np.unique(c[:, 2])) == 1)]


def _tie_witness(k, d, g):
    c, q = g["candidates"][0], int(g["quotas"][0])
    return [("one distinct response on level 0", len(c) > 0 and len(np.unique(c[:, 2])) == 1),
            ("more than 10 x quota candidates", len(c) > 10 * q),
            ("the quota binds", q <= g["n_selected"][0] < len(c))]


def _retry_frame(w=273, h=225):
    """left: texture of amplitude 8 .. 19 in vertical bands (never a corner at threshold 20, plenty at 7 or 4); right: full-range noise"""
    rng = np.random.default_rng(20261017)
    img = np.zeros((h, w), np.int64)
    half = w // 2
    for i, x0 in enumerate(range(0, half, 12)):
        amp = 8 + (i * 3) % 12                                   # 8 .. 19
        img[:, x0:x0 + 12] = 100 + rng.integers(0, amp + 1, (h, min(12, w - x0)))
    img[:, half:] = rng.integers(0, 256, (h, w - half))
    return img.astype(np.uint8)


def _retry_witness(k, d, g):
    retried = sum(st["cells_retried"] for st in g["stats"])
    lo = g["pyramid"][0][:, :120].astype(np.int64)
    return [("at least 10 retried cells", retried >= 10 and g["stats"][0]["cells_retried"] >= 10),
            ("the low-contrast half has amplitude 8 .. 19", 8 <= int(lo.max() - lo.min()) <= 19),
            ("no keypoint below threshold - 1", len(k) > 50 and float(k["response"].min()) >= 19 and all((c[:, 2] >= 19).all() for c in g["candidates"] if len(c))),
            ("no candidate in the low-contrast half of level 0", (g["candidates"][0][:, 0] + 16 >= 120).all())]


def _triangle(img, x, y, direction, height=22, slope=1, v=200):
    """a filled triangle with its one-pixel tip at (x, y), mirror-symmetric about the axis through the tip; slope 1: 90 degree apex, 2: a 53 degree wedge.
    The tip pixel is brighter than the body: on a flat shape the tip and the pixel behind it score the same and suppress each other."""
    for t in range(height):
        half = t // slope
        if direction == "up":                                    # tip on top, body below: m01 > 0
            img[y + t, x - half:x + half + 1] = v
        elif direction == "down":
            img[y - t, x - half:x + half + 1] = v
        elif direction == "left":                                # tip on the left, body to the right: m10 > 0
            img[y - half:y + half + 1, x + t] = v
        else:
            img[y - half:y + half + 1, x - t] = v
    img[y, x] = 255


AXIS_SHAPES = [(50, 40, "up", 1), (120, 40, "up", 2), (190, 70, "down", 1), (260, 70, "down", 2),
               (40, 130, "left", 1), (110, 130, "left", 2), (210, 130, "right", 1), (285, 130, "right", 2)]
AXIS_BLOB = (160, 200)


def _axis_frame(w=320, h=240):
    img = np.full((h, w), 30, np.uint8)
    for x, y, direction, slope in AXIS_SHAPES:
        _triangle(img, x, y, direction, slope=slope)
    bx, by = AXIS_BLOB
    img[by - 1:by + 2, bx - 1:bx + 2] = 200                      # a 3 x 3 blob: symmetric in x and y, both moments zero
    img[by, bx] = 255
    return img


def _axis_witness(k, d, g):
    k0 = k[k["octave"] == 0]
    want = {"up": 90.0, "down": 270.0, "left": 0.0, "right": 180.0}
    out = []
    for direction, a in want.items():
        n = 0
        for x, y, dr, _ in AXIS_SHAPES:
            if dr != direction:
                continue
            on_axis = (k0["x"] == x) if direction in ("up", "down") else (k0["y"] == y)
            near = (np.abs(k0["x"] - x) <= 3) & (np.abs(k0["y"] - y) <= 3)
            n += int((on_axis & near & (k0["angle"] == np.float32(a))).sum())
        out.append(("two tips pointing %s with angle exactly %g" % (direction, a), n >= 2))
    bx, by = AXIS_BLOB
    blob = k0[(k0["x"] == bx) & (k0["y"] == by)]
    out.append(("the symmetric blob is a keypoint with both moments zero (angle exactly 0)", len(blob) == 1 and float(blob["angle"][0]) == 0.0))
    return out


def _byte_range_frame(w=273, h=225):
    """rectangles and single pixels whose values sit at both ends of the byte range: v + t and v - t leave [0, 255] for most centres"""
    rng = np.random.default_rng(20261018)
    vals = np.array([0, 3, 10, 19, 236, 245, 250, 255, 60, 128, 200])
    img = np.full((h, w), 128, np.int64)
    for _ in range(260):
        x, y, bw, bh = int(rng.integers(0, w - 4)), int(rng.integers(0, h - 4)), int(rng.integers(3, 30)), int(rng.integers(3, 30))
        img[y:y + bh, x:x + bw] = int(rng.choice(vals))
    for _ in range(300):
        img[int(rng.integers(0, h)), int(rng.integers(0, w))] = int(rng.choice(vals[:8]))
    return img.astype(np.uint8)


def _byte_range_witness(t):
    def wit(k, d, g):
        c, im = g["candidates"][0], g["pyramid"][0]
        v = im[c[:, 1].astype(np.int64) + 16, c[:, 0].astype(np.int64) + 16].astype(np.int64)
        return [("ten corners with a centre in 255-t+1 .. 255 (v + t > 255)", int((v > 255 - t).sum()) >= 10 and int((v >= 236).sum()) >= 10),
                ("ten corners with a centre in 0 .. t-1 (v - t < 0)", int((v < t).sum()) >= 10 and int((v <= 19).sum()) >= 10),
                ("keypoints on every level", len(np.unique(k["octave"])) == g["quotas"].size)]
    return wit


def _fine_dots_frame(w=320, h=240):
    """single pixels 24 above a flat background: a corner at threshold 20 on level 0; the bilinear reduction by 2 leaves a quarter of the step, so
    levels 1 and 2 have cells (9 x 4, 3 x 1) and not one candidate; level 3 (40 x 30) has no cell.  (A frame whose level 2 finds corners that
    level 1 lacks, a true gap, was tried with soft-edged wedges and did not fire at 80 x 60; the truncated octave set is what is reachable.)"""
    img = np.full((h, w), 60, np.uint8)
    img[24:h - 20:14, 24:w - 20:14] = 84
    return img


def _gap_witness(k, d, g):
    octs = sorted(set(int(o) for o in k["octave"]))
    n_c = [len(c) for c in g["candidates"]]
    with_cells = [l for l, st in enumerate(g["stats"]) if st["grid"][0] > 0 and st["grid"][1] > 0]
    return [("a level with candidates below a level with cells and none", any(n_c[l] > 0 and n_c[l + 1] == 0 and (l + 1) in with_cells for l in range(len(n_c) - 1))),
            ("the octave set has a gap or is truncated", octs != list(range(len(n_c))) and len(octs) >= 1),
            ("level 0 selects keypoints", g["n_selected"][0] > 0)]


def _no_cells_witness(k, d, g):
    grids = [st["grid"] for st in g["stats"]]
    empty = [l for l, gr in enumerate(grids) if gr[0] <= 0 or gr[1] <= 0]
    return [("top levels without a cell column or row", len(empty) >= 2 and empty == list(range(empty[0], len(grids)))),
            ("a level narrower than the two borders", any(im.shape[1] < 32 or im.shape[0] < 32 for im in g["pyramid"])),
            ("lower levels select keypoints", all(g["n_selected"][l] > 0 for l in range(empty[0])) and empty[0] >= 2),
            ("octaves stop where the cells stop", int(k["octave"].max()) == empty[0] - 1)]


def _plain_witness(min_kp, levels):
    return lambda k, d, g: [("at least %d keypoints" % min_kp, len(k) >= min_kp), ("octaves 0 .. %d" % (levels - 1), sorted(set(k["octave"].tolist())) == list(range(levels)))]


def _build():
    C = {}
    C["geom_225x273"] = _case("x: last cell column skipped by -6 (225); y: last cell row skipped by -3 (273)", _edge_frame(41, 225, 273), _geom_witness(225, 273, {
        "12 x 15 cells of 17": lambda st, nc, nr: st["grid"] == (12, 15, 17, 17),
        "last column skipped, views never clipped in x": lambda st, nc, nr: st["cells_skipped_col"] == nr - 1 and st["cols_skipped"] == 1 and set(st["view_w"]) == {23},
        "last row skipped by the -3 rule, the one above clipped to 20": lambda st, nc, nr: st["rows_skipped"] == 1 and set(st["view_h"]) == {23, 20},
        "cells run": lambda st, nc, nr: st["cells_run"] == (nc - 1) * (nr - 1)}))
    C["geom_273x225"] = _case("x: last column skipped, the one before clipped (273); y: last row kept but 6 tall (225)", _edge_frame(42, 273, 225), _geom_witness(273, 225, {
        "15 x 12 cells of 17": lambda st, nc, nr: st["grid"] == (15, 12, 17, 17),
        "no row skipped, the last row's views are 6 tall": lambda st, nc, nr: st["rows_skipped"] == 0 and set(st["view_h"]) == {23, 6} and st["view_h"].count(6) == nc - 1,
        "the 6-tall row finds nothing and is retried": lambda st, nc, nr: st["cells_retried"] >= nc - 1 and all(i < nr - 1 for i, _ in st["cell_of"]),
        "last column skipped, the one before clipped to 20": lambda st, nc, nr: st["cols_skipped"] == 1 and set(st["view_w"]) == {23, 20}}))
    C["geom_209x241"] = _case("x: last view exactly 7 wide (209); y: last row kept, 5 tall, the one above clipped (241)", _edge_frame(43, 209, 241), _geom_witness(209, 241, {
        "11 x 13 cells of 17": lambda st, nc, nr: st["grid"] == (11, 13, 17, 17),
        "last views 7 wide, no column skipped": lambda st, nc, nr: st["cols_skipped"] == 0 and set(st["view_w"]) == {23, 7},
        "the corners of column 189 come from the 7-wide views": lambda st, nc, nr: sum(1 for _, j in st["cell_of"] if j == nc - 1) >= 3,
        "last row kept with 5-tall views, the one above clipped to 22": lambda st, nc, nr: st["rows_skipped"] == 0 and set(st["view_h"]) == {23, 22, 5}}))
    C["geom_241x209"] = _case("x: second-to-last view clipped, last skipped (241); y: last view exactly 7 tall (209)", _edge_frame(44, 241, 209), _geom_witness(241, 209, {
        "13 x 11 cells of 17": lambda st, nc, nr: st["grid"] == (13, 11, 17, 17),
        "last column skipped, the one before clipped to 22": lambda st, nc, nr: st["cols_skipped"] == 1 and set(st["view_w"]) == {23, 22},
        "last views 7 tall, no row skipped": lambda st, nc, nr: st["rows_skipped"] == 0 and set(st["view_h"]) == {23, 7},
        "the corners of row 189 come from the 7-tall views": lambda st, nc, nr: sum(1 for i, _ in st["cell_of"] if i == nr - 1) >= 3}))
    C["levels_without_cells"] = _case("the top levels have nCols == 0 / nRows == 0 (and fall below the border) while lower levels select", synth_image(46, 97, 83), _no_cells_witness,
                                      nfeatures=200, nlevels=8, n_cells=24)
    C["octaves_truncated"] = _case("a level with cells and no candidate above a level with candidates", _fine_dots_frame(), _gap_witness, nfeatures=300, scale=2.0, nlevels=4)
    C["retry_low_contrast"] = _case("cells that find nothing are retried, at the SAME threshold (setThreshold assigns the member to itself)", _retry_frame(), _retry_witness)
    C["periodic_seams"] = _case("equal scores meet across cell seams (both kept) and inside cells (both suppressed)", _periodic(), _seam_witness)
    C["periodic_ties"] = _case("all-equal responses into the octtree, quota far below the candidate count: order and node geometry decide", _periodic(), _tie_witness, nfeatures=30)
    C["axis_angles"] = _case("moments exactly on an axis: angles exactly 0 / 90 / 180 / 270, and atan2(0, 0)", _axis_frame(), _axis_witness, nfeatures=300, nlevels=2, n_cells=30)
    C["byte_range_t20"] = _case("corner centres within t of 0 and 255, threshold 20", _byte_range_frame(), _byte_range_witness(20))
    C["byte_range_t40"] = _case("corner centres within t of 0 and 255, threshold 40", _byte_range_frame(), _byte_range_witness(40), fast_threshold=40)
    rng = np.random.default_rng(20261019)
    C["plain_161x123"] = _case("plain: small odd frame, 16 px cells", synth_image(47, 161, 123), _plain_witness(30, 3), nfeatures=200, nlevels=3)
    C["plain_noise_301x223_s14"] = _case("plain: noise, odd size, scale 1.4, 5 levels", rng.integers(0, 256, (223, 301), dtype=np.uint8), _plain_witness(400, 5), nfeatures=500, scale=1.4, nlevels=5)
    C["plain_320x240_taps256"] = _case("plain: a 256-sum tap set, scale 1.25, 6 levels, 30 px cells", synth_image(48, 320, 240), _plain_witness(300, 6), nfeatures=500, scale=1.25, nlevels=6, n_cells=30,
                                       blur_taps=[16, 34, 50, 56, 50, 34, 16])
    C["plain_640x480"] = _case("plain: the default configuration", synth_image(49, 640, 480), _plain_witness(1000, 8), nfeatures=1000, nlevels=8, n_cells=30)
    return C


CASES = _build()
BATCH_273x225 = ["geom_273x225", "periodic_seams", "retry_low_contrast", "byte_range_t20"]        # one size, one configuration (GEOM); the tie-heavy frame between ordinary ones
VARIANT_CASES = ["periodic_seams", "periodic_ties", "geom_273x225", "geom_209x241", "retry_low_contrast"]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(keypoints, descriptors, debug) of ref_extract.extract for a case: computed once per process, shared by every test, never modified"""
    import ref_extract
    c = CASES[name]
    return ref_extract.extract(c["img"], debug=True, **settings_of(c))


# ---------------------------------------------------------------- front ends: two small stereo pairs, two small colour frames
STEREO = dict(nfeatures=400, scale=1.2, nlevels=5, n_cells=30, fx=500.0, mbf=60.0, n_rows=240)
CAMERA = dict(nfeatures=400, scale=1.2, nlevels=5, n_cells=30)
CAMERA_SCALES = (0.5, 0.75)


def stereo_pairs():
    return [synth_stereo_pair(61, 320, 240), synth_stereo_pair(62, 320, 240)]


def colour_frame(seed, w=480, h=360):
    """a BGR frame: three differently lit renderings of one scene"""
    g = synth_image(seed, w, h).astype(np.int64)
    return np.stack([np.clip(g * 3 // 4 + 20, 0, 255), g, np.clip(g * 5 // 4 - 30, 0, 255)], 2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def stereo_reference(i):
    import ref_extract
    L, R = stereo_pairs()[i]
    return ref_extract.stereo_frontend(L, R, **STEREO)


@functools.lru_cache(maxsize=None)
def camera_reference(scale):
    import ref_extract
    return ref_extract.extract_camera(colour_frame(71), False, scale, **CAMERA)


# ---------------------------------------------------------------- quota arithmetic (no image)
QUOTA_SCALES = (1.1, 1.2, 1.25, 1.4, 1.7, 2.0)
QUOTA_LEVELS = tuple(range(1, 13))
# 1 .. 15000: every small count, then a spread, the product values, and counts found by a search over the whole range with ref_extract.tables
# where cvRound meets an exact .5 (scale 2.0: a level's odd share halves to x.5) or where the rounded shares overshoot nfeatures (last level 0)
QUOTA_NFEATURES = tuple(range(1, 41)) + (50, 63, 64, 65, 77, 100, 127, 128, 129, 200, 255, 256, 300, 500, 511, 512, 750, 1000, 1023, 1024, 1500, 2000, 2047, 2048, 2500, 3000,
                                          4000, 4095, 4096, 5000, 6000, 8000, 8191, 10000, 11600, 12000, 14999, 15000,
                                          444, 1118, 1332, 1385, 1832, 2010, 2393, 3452, 3642, 5701, 12284)
