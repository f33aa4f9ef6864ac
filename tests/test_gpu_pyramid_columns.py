"""The pyramid's column records on the device: the LDS-staged kernels load a lane's window position, byte selectors and coefficient pairs from a
record the plan made per (tile column, lane) instead of deriving them from the x tables.  Every level the device makes against the oracle's pyramid,
byte for byte (debug_level), on every kernel that reads the records:

  level_lds      HS_PYRAMID_NO_FUSE=1: k_resize_level_lds, the records of a level made on its own
  two_levels     chains and the small-batch plan off: k_resize_two_levels, both levels' records requested at the head of the workgroup
  chain_pairs    HS_PYRAMID_CHAIN=2: k_resize_chain, one record per stage, the next stage's requested during the vertical pass
  product        batch 1: the small-batch plan (long chains); batch 3: two-level launches and the chain of the last three levels

with 8 waves per workgroup here and 4 in a child process (HS_PYRAMID_NW8=0 is read once per process), one frame and three frames per call.
Shapes where a record can go wrong: 209 x 97 (the last tile column of a level is one or two pixels wide), 64 x 48 (levels narrower than four lanes'
columns of a tile: most lanes repeat the last column), 613 x 99 (level widths 511, 426, 355, 296, 246, 205, 171: every remainder mod 4, and the first
pair has both widths off a multiple of 4).  Two handles of different sizes alive at once (the records of one plan must not reach the other's
launches), and one handle configured for one size, then another, then the first again.  Images: seeded noise and the 1-px checkerboard."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import hyslam_amd as HS

pytestmark = pytest.mark.gpu
SHAPES = ((209, 97), (64, 48), (613, 99))
LEVELS = 8
NFEAT = 500
PATHS = {
    "level_lds": {"HS_PYRAMID_NO_FUSE": "1"},
    "two_levels": {"HS_PYRAMID_CHAIN": "0", "HS_PYRAMID_DEEP_MAX": "0"},
    "chain_pairs": {"HS_PYRAMID_CHAIN": "2", "HS_PYRAMID_DEEP_MAX": "0"},
    "product": {},
}


def images(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(77 * w + h)
    return [rng.integers(0, 256, (h, w), dtype=np.uint8), (((xx + yy) & 1) * 255).astype(np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)]


def make_reference():
    """{(w, h): (frames, [oracle pyramid per frame])}: computed once, shared by every test, never written to"""
    p = oracle.default_params(NFEAT, 1.2, LEVELS)
    ref = {}
    for w, h in SHAPES:
        frames, pyr = images(w, h), []
        for f in frames:
            lv = [f]
            for l in range(1, LEVELS):
                lv.append(oracle.resize_linear(lv[-1], *oracle.pyramid_size(p, w, h, l)))
            for a in lv:
                a.setflags(write=False)
            pyr.append(lv)
        ref[(w, h)] = (frames, pyr)
    widths = [a.shape[1] for a in ref[(613, 99)][1][0][1:]]
    assert {x & 3 for x in widths} == {0, 1, 2, 3} and widths[0] & 3 and widths[1] & 3, widths
    return ref


@pytest.fixture(scope="module")
def reference():
    return make_reference()


def new_extractor():
    return HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=NFEAT, fScaleFactor=1.2, nLevels=LEVELS))


def check_call(ex, frames, pyr, what):
    ex.extract_batch(frames)
    check_levels(ex, pyr, what)
    return ex.pyramid_launches()


def check_levels(ex, pyr, what):
    for i in range(len(pyr)):
        for l in range(1, LEVELS):
            got = ex.debug_level(i, l)
            assert got.shape == pyr[i][l].shape, (what, i, l, got.shape, pyr[i][l].shape)
            bad = np.argwhere(got != pyr[i][l])
            assert len(bad) == 0, "%s, image %d, level %d: %d bytes differ, first at (row %d, col %d): device %d, oracle %d" % (
                what, i, l, len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], pyr[i][l][tuple(bad[0])])


def check_shape(ex, reference, shape, what):
    """one frame per call (the small-batch plan where it is on) for the noise and the checkerboard, then three frames per call"""
    frames, pyr = reference[shape]
    what = "%s, %dx%d" % ((what,) + shape)
    n1 = [check_call(ex, [frames[i]], [pyr[i]], what + ", batch 1") for i in (0, 1)]
    n3 = check_call(ex, frames, pyr, what + ", batch 3")
    return n1[0], n3


def check_path(reference, path):
    for shape in SHAPES:
        n1, n3 = check_shape(new_extractor(), reference, shape, path)
        if path == "level_lds":
            assert n1 == LEVELS - 1 and n3 == LEVELS - 1, (path, shape, n1, n3)          # a launch per level: nothing fused
        if shape == (613, 99) and path != "level_lds":
            assert n3 < LEVELS - 1, (path, shape, n1, n3)                                   # some launch made more than one level


def check_two_handles(reference, path):
    """two handles of different sizes alive at once, calls interleaved: each one's launches read its own plan's records"""
    a, b = new_extractor(), new_extractor()
    (fa, pa), (fb, pb) = reference[(209, 97)], reference[(613, 99)]
    a.extract_batch(fa)
    b.extract_batch(fb)
    check_levels(a, pa, path + ", first handle after the second one's call")
    check_levels(b, pb, path + ", second handle")
    a.extract_batch([fa[1]])
    b.extract_batch([fb[1]])
    check_levels(b, [pb[1]], path + ", second handle, batch 1")
    check_levels(a, [pa[1]], path + ", first handle, batch 1")


def check_reconfigure(reference, path):
    """one handle, configured for one size, then another, then the first again"""
    ex = new_extractor()
    for shape in ((613, 99), (64, 48), (209, 97), (613, 99)):
        check_shape(ex, reference, shape, path + ", re-configured")


def set_path(monkeypatch, path):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("path", list(PATHS))
def test_every_level_matches_the_oracle(gpu, monkeypatch, reference, path):
    set_path(monkeypatch, path)
    check_path(reference, path)


@pytest.mark.parametrize("path", list(PATHS))
def test_two_handles_of_different_sizes(gpu, monkeypatch, reference, path):
    set_path(monkeypatch, path)
    check_two_handles(reference, path)


@pytest.mark.parametrize("path", list(PATHS))
def test_a_reconfigured_handle(gpu, monkeypatch, reference, path):
    set_path(monkeypatch, path)
    check_reconfigure(reference, path)


def test_four_wave_workgroups_in_a_child_process(gpu):
    """everything above again with 4 waves per workgroup (k_resize_two_levels<4>, k_resize_chain<4>: what launches of many frames run)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    e["HS_PYRAMID_NW8"] = "0"
    e["PYTHONPATH"] = os.pathsep.join([root, os.path.join(root, "tests"), e.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PYRAMID_COLUMNS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


if __name__ == "__main__":
    ref = make_reference()
    for path, env in PATHS.items():
        for k in ("HS_PYRAMID_NO_FUSE", "HS_PYRAMID_CHAIN", "HS_PYRAMID_DEEP_MAX"):
            os.environ.pop(k, None)
        os.environ.update(env)
        check_path(ref, path)
        check_two_handles(ref, path)
        check_reconfigure(ref, path)
    print("PYRAMID_COLUMNS_OK", os.environ.get("HS_PYRAMID_NW8"))
