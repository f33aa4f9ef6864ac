"""GPU: the quadtree kernel's LEVEL instance (kernels_quadtree.hip: eight waves, or four with HS_QT_SMALL_THREADS=256; 512 list entries, level-sized scratch, a histogram pyramid one depth
shallower than the general instance's, four workgroups per CU) against the CPU oracle, bit for bit.

A call of more than 256 (image, level) workgroups without the FAST keys sends the levels [k, L) to it in a launch of their own (run_extract;
HS_QT_SMALL_FROM: -1 = the plan's k, a level = not below that level, L = off).  40 frames of 416 x 320 at 900 features are 320 workgroups and every
level fits the instance, so HS_QT_SMALL_FROM=0 and the default both run every level on it, HS_QT_SMALL_FROM=3 splits the stage into two launches and
HS_QT_SMALL_FROM=8 is the single launch of the general instance.  The frames hold a noise frame (more candidates on level 0 than the instance keeps
in LDS), a constant frame (none) and a frame whose corners all lie in one 40 x 40 px checker patch (nodes deeper than the shallower pyramid: the
point-domain fall-back, counted by hs_debug_quadtree_level_fallbacks)."""
import functools

import numpy as np
import pytest

import oracle
import hyslam_amd as HS
from hyslam_amd import _native as N
from hyslam_amd.synth import synth_image

pytestmark = pytest.mark.gpu
W, H, NFEAT, LEVELS = 416, 320, 900, 8
NOISE, CONST, PATCH = 0, 1, 2


@functools.lru_cache(None)
def frames():
    out = [synth_image(300 + i, W, H) if i % 7 else np.random.default_rng(i).integers(0, 256, (H, W), dtype=np.uint8) for i in range(40)]
    out[CONST] = np.full((H, W), 93, np.uint8)
    patch = np.full((H, W), 128, np.uint8)
    yy, xx = np.mgrid[0:40, 0:40]
    patch[140:180, 200:240] = np.where(((yy // 5) + (xx // 5)) % 2, 230, 20).astype(np.uint8)
    out[PATCH] = patch
    return out


@functools.lru_cache(None)
def refs():
    p = oracle.default_params(NFEAT)
    return [oracle.extract(p, f) for f in frames()]


def same(gk, gd, ok, od):
    assert len(gk) == len(ok), (len(gk), len(ok))
    assert gk.tobytes() == ok.tobytes()
    assert np.array_equal(gd, od)


def extractor(monkeypatch, env):
    for k in ("HS_QT_SMALL_FROM", "HS_QT_POINT_DOMAIN", "HS_QT_SMALL_THREADS", "HS_QT_SMALL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=NFEAT, fScaleFactor=1.2, nLevels=LEVELS))      # the knobs are read here


def check_batch(ex, sel):
    fr, rf = frames(), refs()
    ks, ds = ex.extract_batch([fr[i] for i in sel])
    for j, i in enumerate(sel):
        same(ks[j], ds[j], *rf[i])
    return ks, ds


@pytest.mark.parametrize("env, launches, falls_back", [
    ({"HS_QT_SMALL_FROM": "0"}, 1, True),
    ({}, 1, True),
    ({"HS_QT_SMALL_FROM": "3"}, 2, False),
    ({"HS_QT_SMALL_FROM": "0", "HS_QT_POINT_DOMAIN": "1"}, 1, False),
    ({"HS_QT_SMALL_FROM": "0", "HS_QT_SMALL_THREADS": "256"}, 1, True),
    ({"HS_QT_SMALL_FROM": "8"}, 1, False),
], ids=["from0", "auto", "from3", "from0-point-domain", "from0-256-threads", "off"])
def test_level_instance_equals_the_reference(gpu, monkeypatch, env, launches, falls_back):
    lib = N.lib()
    ex = extractor(monkeypatch, env)
    assert lib.hs_debug_quadtree_level_fallbacks(1) >= 0
    check_batch(ex, range(40))
    assert lib.hs_orb_stage_launches(ex._h, 2) == launches
    n_fall = lib.hs_debug_quadtree_level_fallbacks(1)
    if falls_back:
        assert n_fall > 0, "the checker-patch frame did not leave the count domain on the level instance"
    if env.get("HS_QT_SMALL_FROM") == "8":
        assert n_fall == 0                                           # the instance did not run at all
    # the frames are what the docstring says: level 0 of the noise frame holds more points than any instance keeps in LDS, the constant frame none
    assert len(ex.debug_candidates(NOISE, 0)) > 2048
    assert all(len(ex.debug_candidates(CONST, l)) == 0 for l in range(LEVELS))
    assert len(refs()[PATCH][0]) > 0 and len(refs()[CONST][0]) == 0
    k = refs()[PATCH][0]
    lvl0 = k[k["octave"] == 0]
    assert len(lvl0) > 0 and lvl0["x"].min() >= 195 and lvl0["x"].max() <= 245 and lvl0["y"].min() >= 135 and lvl0["y"].max() <= 185


def test_default_split_is_byte_identical_to_the_general_instance(gpu, monkeypatch):
    a = extractor(monkeypatch, {}).extract_batch(frames())
    b = extractor(monkeypatch, {"HS_QT_SMALL_FROM": str(LEVELS)}).extract_batch(frames())
    for i in range(40):
        assert a[0][i].tobytes() == b[0][i].tobytes() and a[1][i].tobytes() == b[1][i].tobytes(), "frame %d" % i


def test_large_small_large_calls_on_one_handle(gpu, monkeypatch):
    """40 frames (level instance), 2 frames (16 workgroups: the general instance, with the FAST keys), 40 frames again: arrays left non-zero or
    scratch left stale by either instance would show in the next call"""
    ex = extractor(monkeypatch, {"HS_QT_SMALL_FROM": "0"})
    lib = N.lib()
    check_batch(ex, range(40))
    assert lib.hs_orb_stage_launches(ex._h, 2) == 1
    check_batch(ex, [NOISE, PATCH])
    check_batch(ex, [5, CONST])
    check_batch(ex, list(range(39, -1, -1)))


def test_level_instance_under_allocation_poison(gpu, monkeypatch):
    """a fresh handle per byte, every device allocation filled with it before its first use: the instance reads no scratch it has not written"""
    lib = N.lib()
    before = lib.hs_debug_poison_violations()
    seen = []
    try:
        for byte in (0x00, 0xFF, 0xA5):
            assert lib.hs_debug_poison(byte) == N.HS_OK
            ks, ds = check_batch(extractor(monkeypatch, {"HS_QT_SMALL_FROM": "0"}), range(40))
            seen.append(b"".join(k.tobytes() + d.tobytes() for k, d in zip(ks, ds)))
    finally:
        lib.hs_debug_poison(-1)
    assert seen[0] == seen[1] == seen[2]
    assert lib.hs_debug_poison_violations() == before
