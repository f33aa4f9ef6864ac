"""k_preprocess<CN, MODE, ALIGNED> (kernels_preprocess.hip) on the directed table of tests/preprocess_cases.py: hs_preprocess_device on every case with the
case's own source and destination layout, the whole destination buffer compared byte for byte with BOTH CPU references (the oracle and the numpy restatement);
hs_preprocess_size over every width and scale; the call surface (hs_orb_extract_camera_batch, hs_orb_submit_camera_batch / hs_orb_wait) on frames whose
scaled width is no multiple of 4, features against the independent extractor reference; and the refusals include/hyslam_amd.h documents.

One-line faults put into kernels_preprocess.hip on a scratch build, and the first case of test_preprocess_device_on_every_case that caught each:
  1 the area fast path without `+ 2u`                    alignment/cn1_mode1_base0 (also destination, quads, area, random; camera batch area_*)
  2 `(sum + 2) >> 2` in the partial-block branch         destination/mode1_cn4_ow6_tight_pitch, area/cn3_2x3_partial_row (also quads, random)
  3 fast path while `dx0 + 4 <= A.dw`                    area/cn1_7x2_partial_col_fast_path_stops_before_wfull, quads/mode1_cn1_4x1, destination/mode1_cn3_ow8_tight_pitch
  5 no `sx < 0` clamp                                    bilinear/s1.25_cn1_1x5_checker (also grey, random; camera batch bilinear upscales)
  6 `r` and `b` swapped in pre_grey                      alignment/cn3_mode0_base0 (every group; camera batch, tickets)
  7 the store condition without `full_quad`              alignment/cn1_mode0_base0 (row padding overwritten), destination/mode0_cn1_ow5_tight_pitch (next row's first byte)
  4 the right tap always read (no `past` branch)         NOT observable in the output: `past` holds exactly where fx was set to 0, so the extra tap has weight 0; the
                                                         fault only reads CN bytes behind the row.  No byte comparison can catch it.
  8 ALIGNED from the row stride alone                    NOT observable in the output: gfx950 serves a misaligned global dword load, and the aligned path reads exactly
                                                         the quad's own bytes; the alignment/*_base1..3 and *_image_stride_2mod4 cases run it and stay byte-exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import hipmem
import oracle
import preprocess_cases as P
import pyref
import ref_extract as R
import hyslam_amd as HS
from hyslam_amd import _native as N

pytestmark = pytest.mark.gpu
BUF_BYTES = 1 << 20


@pytest.fixture(scope="module")
def ex():
    return HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=P.SURFACE_SETTINGS["nfeatures"], fScaleFactor=P.SURFACE_SETTINGS["scale"],
                                                       nLevels=P.SURFACE_SETTINGS["nlevels"]))


@pytest.fixture(scope="module")
def bufs():
    """one source and one destination block for the whole module; every case is laid out inside them with P.MARGIN bytes to spare on either side"""
    return hipmem.DevBuf(BUF_BYTES), hipmem.DevBuf(BUF_BYTES)


def upload(buf, a):
    assert a.dtype == np.uint8 and a.flags.c_contiguous and a.nbytes <= buf.nbytes
    hipmem._ok(hipmem.hip().hipMemcpy(buf.ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")


def assert_parity(c, rgb, got, want_oracle, want_pyref):
    """the whole destination buffer: the ow x oh rectangles equal both references, every other byte still holds the sentinel"""
    bad = np.nonzero((got != want_oracle) | (got != want_pyref))[0]
    if len(bad):
        i = int(bad[0])
        raise AssertionError("%s rgb=%d (mode %d, %dx%dx%d -> %dx%d): %d bytes differ; first at byte %d = (image, row, column) %r: device %d, oracle %d, restatement %d"
                             % (c["name"], rgb, c["mode"], c["w"], c["h"], c["cn"], c["ow"], c["oh"], len(bad), i, P.locate(c, i), got[i], want_oracle[i], want_pyref[i]))


def run_case(ex, bufs, c, rgb):
    d_src, d_dst = bufs
    upload(d_src, P.src_bytes(c))
    n = P.dst_len(c)
    upload(d_dst, np.full(n, P.SENTINEL_DST, np.uint8))
    ex.preprocess_device(d_src.ptr + P.MARGIN + c["src_off"], c["w"], c["h"], c["src_row"], c["src_img"], c["batch"], c["cn"], rgb, c["scale"],
                         d_dst.ptr + P.MARGIN + c["dst_off"], c["dst_pitch"], c["dst_img"])
    ex.synchronize()
    return d_dst.to_numpy(np.uint8, n)


@pytest.mark.parametrize("group", P.GROUPS)
def test_preprocess_device_on_every_case(gpu, ex, bufs, group):
    cases = P.by_group(group)
    assert cases
    for c in cases:
        for rgb in c["orders"]:
            frames = [P.frame_of(c, i) for i in range(c["batch"])]
            a = [oracle.preprocess(f, rgb, c["scale"]) for f in frames]
            b = [pyref.preprocess(f, rgb, c["scale"]) for f in frames]
            assert a[0].shape == b[0].shape == (c["oh"], c["ow"]), c["name"]
            assert_parity(c, rgb, run_case(ex, bufs, c, rgb), P.dst_bytes(c, a), P.dst_bytes(c, b))


def test_preprocess_size_every_width_and_scale(gpu):
    """hs_preprocess_size == cvRound of the double product, half to even, for every width from 1 to 4096 (as width and as height) at every scale of the table —
    0.5, 0.25, 0.75, 1.25 and 1.5 have exact ties among them"""
    lib = N.lib()
    w = np.arange(1, 4097)
    ties = 0
    for s in P.all_scales():
        prod = w.astype(np.float64) * np.float64(np.float32(s))
        want = pyref.cv_round(prod)
        ties += int((prod - np.floor(prod) == 0.5).sum())
        ow, oh = C.c_int32(), C.c_int32()
        for i in range(len(w)):
            lib.hs_preprocess_size(int(w[i]), int(w[len(w) - 1 - i]), C.c_float(s), C.byref(ow), C.byref(oh))
            assert (ow.value, oh.value) == (want[i], want[len(w) - 1 - i]), (s, int(w[i]))
    assert ties > 5000


# ---- the call surface ------------------------------------------------------------------------------------------------------------------------
def surface_frames(c):
    f = P.surface_frame(c)
    return [f, np.ascontiguousarray(f[::-1, ::-1])]                   # two different frames: the second one sits one image stride into the level-0 buffer


@functools.lru_cache(maxsize=None)
def surface_reference(name):
    """[(grey, keypoints, descriptors)] per frame from the restatements alone: pyref.preprocess, then ref_extract.extract"""
    c = next(x for x in P.SURFACE if x["name"] == name)
    out = []
    for f in surface_frames(c):
        g = pyref.preprocess(f, c["rgb"], c["scale"])
        assert np.array_equal(g, oracle.preprocess(f, c["rgb"], c["scale"])), name
        k, d = R.extract(g, P.SURFACE_SETTINGS["nfeatures"], P.SURFACE_SETTINGS["scale"], P.SURFACE_SETTINGS["nlevels"])
        out.append((g, k, d))
    return out


def assert_features(what, gk, gd, rk, rd):
    assert len(gk) == len(rk), (what, len(gk), len(rk))
    assert gk.tobytes() == rk.tobytes() and np.array_equal(gd, rd), what


@pytest.mark.parametrize("name", [c["name"] for c in P.SURFACE])
def test_camera_batch_grey_and_features(gpu, ex, name):
    """hs_orb_extract_camera_batch: the grey frames it returns equal both references, the features equal the independent extractor reference on that grey
    frame.  ow % 4 != 0: the internal call pads its last quad into the handle's level-0 buffer (zeros behind column ow); neither output may show it."""
    c = next(x for x in P.SURFACE if x["name"] == name)
    ref = surface_reference(name)
    k, d, grey = ex.extract_camera_batch(surface_frames(c), c["rgb"], c["scale"], want_grey=True)
    assert [g.shape for g in grey] == [(c["oh"], c["ow"])] * 2
    for i, (g, rk, rd) in enumerate(ref):
        if not np.array_equal(grey[i], g):
            y, x = np.argwhere(grey[i] != g)[0]
            raise AssertionError("%s frame %d: grey differs first at row %d column %d: device %d, references %d" % (name, i, y, x, grey[i][y, x], g[y, x]))
        assert_features((name, i), k[i], d[i], rk, rd)
    assert sum(len(rk) for _, rk, _ in ref) > 20, "the frame must have corners for the feature comparison to mean anything"


@pytest.mark.parametrize("first,second", P.SURFACE_PAIRS)
def test_two_camera_tickets_in_flight(gpu, ex, first, second):
    """hs_orb_submit_camera_batch / hs_orb_wait: two tickets in flight that differ in channels and scale (each slot has its own raw buffer; the kernel
    instantiation switches between them on one handle), then the first kind again while the second is still in flight"""
    ca, cb = (next(x for x in P.SURFACE if x["name"] == n) for n in (first, second))
    fa, fb = surface_frames(ca), surface_frames(cb)
    t1 = ex.submit_camera_batch(fa, ca["rgb"], ca["scale"])
    t2 = ex.submit_camera_batch(fb, cb["rgb"], cb["scale"])
    r1 = ex.wait(t1)
    t3 = ex.submit_camera_batch(fa[::-1], ca["rgb"], ca["scale"])
    r2, r3 = ex.wait(t2), ex.wait(t3)
    for what, (n, k, d, _, _), ref in ((first, r1, surface_reference(first)), (second, r2, surface_reference(second)), (first + " again", r3, surface_reference(first)[::-1])):
        for i, (_, rk, rd) in enumerate(ref):
            assert_features((what, i), k[i, :n[i]], d[i, :n[i]], rk, rd)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
REFUSED = {                                                           # name: (w, h, row stride, channels, scale, grey row stride)
    "two_channels": (16, 8, 64, 2, 1.0, 16),
    "no_channels": (16, 8, 64, 0, 1.0, 16),
    "five_channels": (16, 8, 80, 5, 1.0, 16),
    "empty_output": (4, 4, 4, 1, 0.1, 16),                           # cvRound(0.4) = 0
    "empty_output_height_only": (16, 1, 16, 1, 0.25, 16),            # 4 x cvRound(0.25) = 4 x 0
    "row_stride_below_a_row": (16, 8, 47, 3, 1.0, 16),
    "width_above_32768": (32769, 1, 32772, 1, 0.25, 8196),
    "height_above_32768": (1, 32769, 4, 1, 0.25, 4),
    "scaled_width_above_16384": (16385, 1, 16388, 1, 1.0, 16388),
    "grey_row_stride_below_ow": (16, 8, 16, 1, 1.0, 15),
    "scale_zero": (16, 8, 16, 1, 0.0, 16),
    "scale_above_16": (16, 8, 16, 1, 16.5, 1024),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_preprocess_device_refusals(gpu, ex, bufs, name):
    """every documented refusal returns HS_ERR_INVALID, leaves the destination untouched and the handle usable"""
    w, h, row, cn, scale, gpitch = REFUSED[name]
    d_src, d_dst = bufs
    sentinel = np.full(BUF_BYTES, P.SENTINEL_DST, np.uint8)
    upload(d_dst, sentinel)
    with pytest.raises(HS.HsError) as e:
        ex.preprocess_device(d_src.ptr, w, h, row, row * h, 1, cn, True, scale, d_dst.ptr, gpitch, 0)
    assert e.value.status == N.HS_ERR_INVALID
    ex.synchronize()
    assert np.array_equal(d_dst.to_numpy(np.uint8, BUF_BYTES), sentinel), "a refused call wrote to the destination"
    c = P.CASES["destination/mode1_cn4_ow6_tight_pitch"]
    f = [P.frame_of(c, 0)]
    assert_parity(c, True, run_case(ex, bufs, c, True), P.dst_bytes(c, [oracle.preprocess(f[0], True, c["scale"])]), P.dst_bytes(c, [pyref.preprocess(f[0], True, c["scale"])]))


def test_camera_batch_refusals(gpu, ex):
    """the same conditions at the two host-frame entry points, called through the C ABI (the Python wrapper would refuse some of them itself)"""
    lib, hdl = ex._lib, ex._h
    frame = P.surface_frame(P.SURFACE[0])
    cap = 4096
    kps, desc, n = np.zeros(cap, N.KP_DTYPE), np.full((cap, 32), 0x5A, np.uint8), np.full(1, -7, np.int32)
    grey = np.full(frame.shape[0] * frame.shape[1], P.SENTINEL_DST, np.uint8)
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    h, w = frame.shape
    for what, (cw, ch, row, cn, scale) in dict(two_channels=(w // 2, h, w, 2, 1.0), five_channels=(w // 5, h, w, 5, 1.0), empty_output=(w, h, w, 1, 0.001),
                                               row_stride_below_a_row=(w, h, w - 1, 1, 1.0), width_above_32768=(32769, 1, 32769, 1, 0.01),
                                               height_above_32768=(1, 32769, 1, 1, 0.01)).items():
        pp = N.PreprocessParams(cn, 1, scale, 0)
        rc = lib.hs_orb_extract_camera_batch(hdl, ptrs, 1, cw, ch, row, C.byref(pp), vp(kps), vp(desc), cap, vp(n), vp(grey))
        assert rc == N.HS_ERR_INVALID, (what, rc)
        assert n[0] == -7 and (desc == 0x5A).all() and (grey == P.SENTINEL_DST).all() and not kps.tobytes().strip(b"\0"), what
        t = C.c_int32(-7)
        rc = lib.hs_orb_submit_camera_batch(hdl, ptrs, 1, cw, ch, row, C.byref(pp), None, C.byref(t))
        assert rc == N.HS_ERR_INVALID and t.value <= 0, (what, rc, t.value)
        # the handle still works, through both entry points
        name = P.SURFACE[0]["name"]
        (g, rk, rd) = surface_reference(name)[0]
        k, d, gg = ex.extract_camera_batch([frame], True, 1.0, want_grey=True)
        assert np.array_equal(gg[0], g), what
        assert_features((what, "after the refusal"), k[0], d[0], rk, rd)
    nn, k, d, _, _ = ex.wait(ex.submit_camera_batch([frame], True, 1.0))
    assert_features("ticket after the refusals", k[0, :nn[0]], d[0, :nn[0]], *surface_reference(P.SURFACE[0]["name"])[0][1:])
