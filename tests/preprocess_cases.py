"""Directed cases for ImageProcessing::PreProcessImg on the device (kernels_preprocess.hip: k_preprocess<CN, MODE, ALIGNED>), shared by the CPU
reference test (test_preprocess_ref.py) and the GPU edge test (test_gpu_preprocess_edges.py).  Generated deterministically from fixed seeds.

A case is a dict:
  name, group                     the name says which kernel branch the case exists for
  w, h, cn, scale                 the source frame and the camera's scale (a Python float that is exactly a float32)
  orders                          the colour orders to run (rgb = True / False; one order for cn == 1, where it cannot matter)
  src_off, src_row, src_img, batch    source layout in bytes: image i at base + src_off + i * src_img, rows src_row apart
  dst_off, dst_pitch, dst_img     destination layout likewise
  ow, oh, mode                    what the table expects of the size (cvRound) and the path (0 copy, 1 the 2x2 area path, 2 bilinear); stated here from the
                                  specification and checked against the library / the oracle by the tests
  frames                          uint8 (batch, h, w, cn): the source bytes

`base` is an address that is a multiple of 256 (the test's allocation plus a margin), so src_off / dst_off ARE the address modulo 4.
"""
import numpy as np

import pyref

SENTINEL_DST = 0xAB          # pre-fill of the destination: every byte outside the ow x oh rectangles must still hold it
SENTINEL_GAP = 0xEE          # fill of the source bytes between rows and images: the result must not depend on them
MARGIN = 256                 # bytes the tests keep free in front of and behind every laid-out buffer

F32 = np.float32
NEXT_BELOW_HALF = float(np.nextafter(F32(0.5), F32(0)))      # 0.49999997: 1 / scale is 2 + 1.2e-7 -> bilinear
NEXT_ABOVE_HALF = float(np.nextafter(F32(0.5), F32(1)))      # 0.50000006: 1 / scale is 2 - 2.4e-7 -> bilinear
BILINEAR_SCALES = [float(F32(s)) for s in (0.75, 0.4, 0.3333, 0.25, 1.25, 1.5, 2.0, 3.0)] + [NEXT_BELOW_HALF, NEXT_ABOVE_HALF]
SAME_SIZE_SCALE = float(F32(0.999))                          # 67 x 35 stays 67 x 35: a copy
KEEP_ONE_SCALE = float(F32(0.99))                            # 37 stays 37, 60 becomes 59: bilinear with an identity-sized axis
AREA_SIZES = (2, 3, 5, 6, 7, 9, 10, 11, 13, 17, 18, 19)
GROUPS = ("alignment", "destination", "quads", "area", "bilinear", "copy", "grey", "random")


def colour_frame(seed, w, h, cn):
    """a structured grey scene per channel (different seeds: the channels differ), so that the grey result has corners"""
    from hyslam_amd.synth import synth_image
    if cn == 1:
        return synth_image(seed, w, h)
    chans = [synth_image(seed + 7 * k, w, h) for k in range(3)]
    if cn == 4:
        chans.append(np.full((h, w), 200, np.uint8))
    return np.ascontiguousarray(np.stack(chans, axis=2))


def out_size(w, h, scale):
    """cv::resize's dsize for fx = fy = scale: cvRound of the double product, half to even"""
    inv = np.float64(F32(scale))
    return int(pyref.cv_round(np.float64(w) * inv)), int(pyref.cv_round(np.float64(h) * inv))


def mode_of(w, h, scale):
    """0 copy (the size does not change), 1 INTER_AREA's 2x2 fast path (1 / scale is 2 within DBL_EPSILON), 2 bilinear"""
    if out_size(w, h, scale) == (w, h):
        return 0
    s = 1.0 / np.float64(F32(scale))
    return 1 if abs(s - 2.0) < np.finfo(np.float64).eps else 2


def src_for(o, scale):
    """the smallest source extent whose scaled extent is o"""
    for s in range(1, 1 << 16):
        if out_size(s, s, scale)[0] == o:
            return s
    raise ValueError((o, scale))


def up4(v):
    return (v + 3) & ~3


# ---- content -------------------------------------------------------------------------------------------------------------------------------
def _grey_triples():
    """(c0, c1, c2) whose weighted sum lands next to the rounding term of cvtColor in either colour order, on both sides: the remainder of
    (R 4899 + G 9617 + B 1868) modulo 2^14 is within 64 of 2^13, so `+ (1 << 13)` decides the grey value and a truncating sum is one short"""
    r = np.arange(0, 256, 5, dtype=np.int64)[:, None, None]
    g = np.arange(256, dtype=np.int64)[None, :, None]
    b = np.arange(256, dtype=np.int64)[None, None, :]
    rem = (r * 4899 + g * 9617 + b * 1868) & 16383
    out = []
    for lo, hi in ((8192, 8192 + 64), (8192 - 64, 8192)):
        i = np.argwhere((rem >= lo) & (rem < hi) & (r != b))
        i = i[:: max(1, len(i) // 40)][:40]
        out.append(np.stack([i[:, 0] * 5, i[:, 1], i[:, 2]], axis=1))
    return np.concatenate(out).astype(np.uint8)


_PURE = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0], [255, 255, 0], [0, 255, 255], [255, 0, 255],
                  [1, 0, 0], [0, 0, 1], [254, 255, 255], [255, 255, 254], [128, 127, 129]], np.uint8)


def content(kind, rng, batch, h, w, cn):
    """uint8 (batch, h, w, cn).  random; checker (0 / 255 in single pixels, phase differs per channel); ramp (columns 0..255 and back); area_sharp
    (every full 2x2 block sums to 2 mod 4, so (sum + 2) >> 2 is one above truncation; every two-sample partial block has an odd sum, so its float
    mean ends in .5 and half-to-even shows on alternating parities); grey_sharp (pure, saturated and rounding-decided pixels; alpha random)"""
    f = rng.integers(0, 256, (batch, h, w, cn), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "random":
        pass
    elif kind == "checker":
        for k in range(cn):
            f[..., k] = np.where((yy + xx + k) & 1, 255, 0)
    elif kind == "ramp":
        for k in range(cn):
            v = (xx * 37 + k * 85) % 510
            f[..., k] = np.where(v > 255, 510 - v, v)
    elif kind == "area_sharp":
        a = f.astype(np.int64)
        for y0 in range(0, h, 2):
            for x0 in range(0, w, 2):
                blk = a[:, y0:y0 + 2, x0:x0 + 2, :]
                n = blk.shape[1] * blk.shape[2]
                if n == 1:
                    continue
                rest = blk.reshape(batch, n, cn)[:, 1:, :].sum(axis=1)
                want = 2 if n == 4 else 1 + 2 * (((x0 + y0) >> 1) & 1)         # n == 2: sums 1 and 3 modulo 4 -> means k + .5 with k even and odd
                a[:, y0, x0, :] = (a[:, y0, x0, :] & 0xFC) + ((want - rest) % 4)
        f = a.astype(np.uint8)
    elif kind == "grey_sharp":
        px = np.concatenate([_PURE, _grey_triples()])
        idx = (np.arange(batch * h * w) * 7 + int(rng.integers(0, len(px)))) % len(px)
        f[..., :min(cn, 3)] = px[idx].reshape(batch, h, w, 3)[..., :min(cn, 3)]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(f)


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
CASES = {}
_seed = [20240]


def make(group, name, w, h, cn, scale, kind="random", batch=1, src_off=0, src_row=None, src_img=None, dst_off=0, dst_pitch=None, dst_img=None, mode=None):
    """defaults: everything aligned — source rows up4(w cn) apart, images packed; destination pitch up4(ow), images packed"""
    scale = float(F32(scale))
    ow, oh = out_size(w, h, scale)
    assert ow >= 1 and oh >= 1, (name, "the table must not hold an empty output size")
    src_row = up4(w * cn) if src_row is None else src_row
    src_img = src_row * h if src_img is None else src_img
    dst_pitch = up4(ow) if dst_pitch is None else dst_pitch
    dst_img = dst_pitch * oh if dst_img is None else dst_img
    assert src_row >= w * cn and src_img >= src_row * (h - 1) + w * cn and dst_pitch >= ow and dst_img >= dst_pitch * (oh - 1) + ow, name
    m = mode_of(w, h, scale)
    assert mode is None or m == mode, (name, "expected mode %r, the specification gives %d" % (mode, m))
    _seed[0] += 1
    rng = np.random.default_rng(_seed[0])
    full = "%s/%s" % (group, name)
    assert full not in CASES, full
    CASES[full] = dict(name=full, group=group, w=w, h=h, cn=cn, scale=scale, orders=(True, False) if cn > 1 else (True,), batch=batch,
                       src_off=src_off, src_row=src_row, src_img=src_img, dst_off=dst_off, dst_pitch=dst_pitch, dst_img=dst_img,
                       ow=ow, oh=oh, mode=m, frames=content(kind, rng, batch, h, w, cn))
    return CASES[full]


_MODE_SCALE = ((0, 1.0), (1, 0.5), (2, 0.75))


def _alignment():
    # ALIGNED = ((base | row stride | image stride) & 3) == 0 picks dword or byte loads.  38 x 10: full quads and a partial one at every mode.
    for cn in (1, 3, 4):
        for mode, scale in _MODE_SCALE:
            t = "cn%d_mode%d" % (cn, mode)
            row = up4(38 * cn)
            for off in range(4):                                     # off 0: ALIGNED = true; 1..3: a misaligned base alone must select byte loads
                make("alignment", "%s_base%d" % (t, off), 38, 10, cn, scale, src_off=off, mode=mode)
            make("alignment", "%s_odd_row_stride" % t, 38, 10, cn, scale, src_row=row + 1, mode=mode)
            # rows aligned, the image stride 2 modulo 4: image 0 is aligned, image 1 is not — ALIGNED must be false for the whole launch
            make("alignment", "%s_image_stride_2mod4" % t, 38, 10, cn, scale, batch=2, src_img=row * 10 + 2, mode=mode)


def _destination():
    # the store: a dword when the quad is full and the row base + column is a multiple of 4, bytes otherwise; never past ow
    for mi, (mode, scale) in enumerate(_MODE_SCALE):
        for j, ow in enumerate((5, 6, 7, 9, 10, 11, 8)):
            cn = (1, 3, 4)[(j + mi) % 3]
            w, h = src_for(ow, scale), src_for(3, scale)
            t = "mode%d_cn%d_ow%d" % (mode, cn, ow)
            # tight pitch: a padded dword store of one row's tail would land on the first bytes of the next row
            make("destination", "%s_tight_pitch" % t, w, h, cn, scale, dst_pitch=ow, mode=mode)
            make("destination", "%s_pitch_ow_plus1" % t, w, h, cn, scale, dst_pitch=ow + 1, mode=mode)
            for off in range(4):                                     # base modulo 4 with an aligned pitch, then with a tight one
                make("destination", "%s_base%d" % (t, off), w, h, cn, scale, dst_off=off, mode=mode)
                make("destination", "%s_base%d_tight" % (t, off), w, h, cn, scale, dst_off=off, dst_pitch=ow, mode=mode)
            # three images further apart than oh * pitch: the gap between images stays untouched
            make("destination", "%s_batch3_gap" % t, w, h, cn, scale, batch=3, dst_pitch=ow + 2, dst_img=(ow + 2) * 3 + 13, mode=mode)


def _quads():
    # a lane makes 4 pixels, a workgroup 256 x 4: the row's last partial quad, the second and fifth workgroup in x, the second workgroup in y
    for mode, scale in ((0, 1.0), (1, 0.5), (2, 0.4)):
        j = 0
        for ow in (1, 2, 3, 4, 5, 255, 256, 257, 1025):
            for oh in (1, 2, 3, 4, 5):
                cn = (1, 3, 4)[j % 3]
                j += 1
                make("quads", "mode%d_cn%d_%dx%d" % (mode, cn, ow, oh), src_for(ow, scale), src_for(oh, scale), cn, scale, mode=mode)
        for cn in (3, 4):                                            # every colour layout beyond the first workgroup in x
            for ow in (257, 1025):
                make("quads", "mode%d_cn%d_%dx5_wide" % (mode, cn, ow), src_for(ow, scale), src_for(5, scale), cn, scale, kind="ramp", mode=mode)


def _area():
    # scale 0.5.  w odd with cvRound up (3, 7, 11, 19): a partial column of two samples; down (5, 9, 13, 17): the last column belongs to no block;
    # likewise rows; both odd and up: the one-sample corner.  7 (and 15, 23): ow = 4 k is a full quad but w >> 1 = 4 k - 1, the aligned fast path must
    # stop one quad early.
    j = 0
    for w in AREA_SIZES + (15, 23):
        for h in AREA_SIZES:
            cn = (1, 3, 4)[j % 3]
            j += 1
            tag = []
            if w & 1:
                tag.append("partial_col" if out_size(w, h, 0.5)[0] * 2 > w else "dropped_col")
            if h & 1:
                tag.append("partial_row" if out_size(w, h, 0.5)[1] * 2 > h else "dropped_row")
            if len(tag) == 2 and tag[0] == "partial_col" and tag[1] == "partial_row":
                tag = ["one_sample_corner"]
            if w in (7, 15, 23):
                tag.append("fast_path_stops_before_wfull")
            make("area", "cn%d_%dx%d_%s" % (cn, w, h, "_".join(tag) or "full_blocks"), w, h, cn, 0.5, kind="area_sharp", mode=1)
    for cn in (1, 3, 4):                                             # the same classes with random bytes, and 0 / 255 (sums 510 and 1020: saturation is not reached, 255 is)
        for (w, h) in ((7, 7), (5, 9), (19, 3), (18, 6), (23, 11)):
            make("area", "cn%d_%dx%d_random" % (cn, w, h), w, h, cn, 0.5, mode=1)
            make("area", "cn%d_%dx%d_checker" % (cn, w, h), w, h, cn, 0.5, kind="checker", mode=1)


def _bilinear():
    # clamps: sx < 0 (left border of every upscale), sx >= sw - 1 with the right tap not read (`past`), rows clipped above and below; source width 1
    # or height 1: every tap clamps; 2 x 2: both at once.  One-row outputs and outputs narrower than 4 come from the small sources.
    kinds = ("checker", "ramp", "random")
    j = 0
    for scale in BILINEAR_SCALES:
        down = scale < 1
        sizes = ((7, 5), (13, 9), (37, 11), (64, 6), (9, 33), (6, 4)) if down else ((1, 5), (5, 1), (2, 2), (7, 5), (21, 3), (1, 1))
        for (w, h) in sizes:
            if mode_of(w, h, scale) != 2:                           # (1 x 1 at 1.25 stays 1 x 1: that is the copy group's)
                continue
            for cn in (1, 3, 4):
                make("bilinear", "s%.8g_cn%d_%dx%d_%s" % (scale, cn, w, h, kinds[j % 3]), w, h, cn, scale, kind=kinds[j % 3], mode=2)
                j += 1
    for cn in (1, 3, 4):
        # one dimension keeps its size, the other shrinks: the bilinear path with an identity-sized axis (fx == 0 for every column, or fy for every row)
        make("bilinear", "keep_width_cn%d_37x60" % cn, 37, 60, cn, KEEP_ONE_SCALE, kind="checker", mode=2)
        make("bilinear", "keep_height_cn%d_60x37" % cn, 60, 37, cn, KEEP_ONE_SCALE, kind="ramp", mode=2)
        make("bilinear", "keep_height1_cn%d_37x1" % cn, 37, 1, cn, 0.75, kind="checker", mode=2)
        make("bilinear", "keep_width1_cn%d_1x9" % cn, 1, 9, cn, 1.25, kind="ramp", mode=2)


def _copy():
    for cn in (1, 3, 4):
        make("copy", "scale1_cn%d_67x35" % cn, 67, 35, cn, 1.0, mode=0)
        make("copy", "same_size_0.999_cn%d_67x35" % cn, 67, 35, cn, SAME_SIZE_SCALE, mode=0)      # a scale other than 1 that keeps both dimensions: no resampling
        make("copy", "same_size_1.25_cn%d_1x1" % cn, 1, 1, cn, 1.25, mode=0)
        make("copy", "same_size_1.001_cn%d_40x3" % cn, 40, 3, cn, 1.001, kind="checker", mode=0)


def _grey():
    # cvtColor: (R 4899 + G 9617 + B 1868 + (1 << 13)) >> 14 in both colour orders; alpha is random and must not matter
    for cn in (3, 4):
        make("grey", "copy_cn%d_sharp" % cn, 53, 4, cn, 1.0, kind="grey_sharp", mode=0)
        make("grey", "copy_cn%d_sharp_odd_stride" % cn, 53, 4, cn, 1.0, kind="grey_sharp", src_row=53 * cn + 1, mode=0)
        make("grey", "bilinear_upscale_cn%d_sharp" % cn, 13, 3, cn, 2.0, kind="grey_sharp", mode=2)
        c = make("grey", "area_cn%d_sharp_flat_blocks" % cn, 54, 4, cn, 0.5, kind="grey_sharp", mode=1)
        c["frames"][:, 1::2] = c["frames"][:, 0::2]                 # every 2x2 block holds one pixel four times: the mean is the pixel itself
        c["frames"][:, :, 1::2] = c["frames"][:, :, 0::2]


def _random():
    rng = np.random.default_rng(77001)
    scales = [1.0, 0.5, 0.5, 0.5, SAME_SIZE_SCALE, KEEP_ONE_SCALE] + BILINEAR_SCALES
    for i in range(200):
        scale = scales[int(rng.integers(0, len(scales)))]
        cn = (1, 3, 4)[int(rng.integers(0, 3))]
        while True:
            w, h = int(rng.integers(1, 97)), int(rng.integers(1, 65))
            ow, oh = out_size(w, h, scale)
            if ow >= 1 and oh >= 1:
                break
        batch = int(rng.integers(1, 4))
        row = w * cn + int(rng.integers(0, 9))
        if rng.integers(0, 2):
            row = up4(row)
        img = row * h + int(rng.integers(0, 7))
        pitch = ow + int(rng.integers(0, 6))
        make("random", "%03d_cn%d_%dx%d_s%.8g" % (i, cn, w, h, scale), w, h, cn, scale, kind=("random", "checker", "ramp", "area_sharp")[int(rng.integers(0, 4))],
             batch=batch, src_off=int(rng.integers(0, 4)) * int(rng.integers(0, 2)), src_row=row, src_img=img,
             dst_off=int(rng.integers(0, 4)), dst_pitch=pitch, dst_img=pitch * oh + int(rng.integers(0, 9)))


for _g in (_alignment, _destination, _quads, _area, _bilinear, _copy, _grey, _random):
    _g()


def by_group(group):
    return [c for c in CASES.values() if c["group"] == group]


def all_scales():
    """every scale the table uses, and the exact ties of cvRound they produce (0.5, 0.25, 0.75, 1.25, 1.5 on suitable widths)"""
    return sorted({c["scale"] for c in CASES.values()} | {c["scale"] for c in SURFACE})


# ---- layouts -------------------------------------------------------------------------------------------------------------------------------
def src_bytes(c):
    """the source buffer as the device sees it: MARGIN sentinel bytes, then the frames at src_off with their strides, gaps filled with SENTINEL_GAP,
    then a margin again.  The first frame byte is at index MARGIN + src_off."""
    n = MARGIN + c["src_off"] + (c["batch"] - 1) * c["src_img"] + (c["h"] - 1) * c["src_row"] + c["w"] * c["cn"] + MARGIN
    buf = np.full(up4(n), SENTINEL_GAP, np.uint8)
    rb = c["w"] * c["cn"]
    for i in range(c["batch"]):
        for y in range(c["h"]):
            o = MARGIN + c["src_off"] + i * c["src_img"] + y * c["src_row"]
            buf[o:o + rb] = c["frames"][i, y].reshape(-1)
    return buf


def dst_len(c):
    return up4(MARGIN + c["dst_off"] + (c["batch"] - 1) * c["dst_img"] + (c["oh"] - 1) * c["dst_pitch"] + c["ow"] + MARGIN)


def dst_bytes(c, greys):
    """the destination buffer as it must look afterwards: SENTINEL_DST everywhere but in the ow x oh rectangles, which hold `greys` (batch, oh, ow)"""
    buf = np.full(dst_len(c), SENTINEL_DST, np.uint8)
    for i in range(c["batch"]):
        for y in range(c["oh"]):
            o = MARGIN + c["dst_off"] + i * c["dst_img"] + y * c["dst_pitch"]
            buf[o:o + c["ow"]] = greys[i][y]
    return buf


def locate(c, index):
    """byte index of the destination buffer -> (image, row, column) or a word for the bytes outside every rectangle"""
    o = index - MARGIN - c["dst_off"]
    if o < 0:
        return "in front of image 0"
    i = min(o // c["dst_img"], c["batch"] - 1)
    y, x = divmod(o - i * c["dst_img"], c["dst_pitch"])
    if y >= c["oh"]:
        return "behind image %d" % i
    return (int(i), int(y), int(x)) if x < c["ow"] else "row padding of image %d row %d, column %d" % (i, y, x)


def frame_of(c, i):
    f = c["frames"][i]
    return f[:, :, 0] if c["cn"] == 1 else f


# ---- the call surface: camera frames in, features out.  Output sizes of at least 64 x 48 with ow % 4 in {1, 2, 3}: there the internal call writes its
# padded quad into the handle's own level-0 buffer, and neither the returned grey nor the features may show the pad.
SURFACE_SETTINGS = dict(nfeatures=300, scale=1.2, nlevels=3)
SURFACE = [dict(name=n, w=w, h=h, cn=cn, rgb=rgb, scale=float(F32(s)), seed=900 + i) for i, (n, w, h, cn, rgb, s) in enumerate((
    ("copy_grey_201x141", 201, 141, 1, True, 1.0),
    ("copy_rgb_202x142", 202, 142, 3, True, 1.0),
    ("copy_bgra_203x143", 203, 143, 4, False, 1.0),
    ("same_size_grey_199x141", 199, 141, 1, True, SAME_SIZE_SCALE),
    ("area_bgr_402x282_to_201x141", 402, 282, 3, False, 0.5),
    ("area_rgba_405x285_to_202x142_dropped", 405, 285, 4, True, 0.5),
    ("area_grey_406x286_to_203x143", 406, 286, 1, True, 0.5),
    ("area_rgb_403x283_to_202x142_partial", 403, 283, 3, True, 0.5),
    ("bilinear_rgb_268x188_to_201x141", 268, 188, 3, True, 0.75),
    ("bilinear_bgra_161x113_to_201x141", 161, 113, 4, False, 1.25),
    ("bilinear_grey_101x71_to_202x142", 101, 71, 1, True, 2.0),
    ("bilinear_bgr_67x47_to_201x141", 67, 47, 3, False, 3.0),
    ("below_half_rgb_410x284_to_205x142", 410, 284, 3, True, NEXT_BELOW_HALF),
))]
for _c in SURFACE:
    _c["ow"], _c["oh"] = out_size(_c["w"], _c["h"], _c["scale"])
    assert _c["ow"] >= 64 and _c["oh"] >= 48 and _c["ow"] % 4 != 0, _c["name"]
assert {c["ow"] % 4 for c in SURFACE} == {1, 2, 3}
# tickets that are in flight together: same level-0 size (one workspace geometry), different channels and scale
SURFACE_PAIRS = (("copy_grey_201x141", "area_bgr_402x282_to_201x141"), ("area_rgba_405x285_to_202x142_dropped", "bilinear_grey_101x71_to_202x142"),
                 ("bilinear_bgra_161x113_to_201x141", "copy_grey_201x141"))


def surface_frame(c):
    return colour_frame(c["seed"], c["w"], c["h"], c["cn"])
