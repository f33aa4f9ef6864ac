"""The pyramid's LDS-staged kernels — horizontal sums, vertical combine (pyr_vquad), the row loops around them, and the order in which
k_resize_two_levels requests its x-table records — on each of the three kernels: every level the device made against the oracle's pyramid, byte
for byte.  Small frames that reach the edges the large parity cases do not single out.

Paths (the launch count of the call says which plan ran; asserted at 209 x 97, where every plan is possible):
  k_resize_level_lds    HS_PYRAMID_NO_FUSE=1: one launch per level
  k_resize_two_levels   chains and the small-batch plan switched off: pairs of levels, so fewer launches than levels
  k_resize_chain        the small-batch plan (calls of <= 2 frames): one or two long chains; and HS_PYRAMID_CHAIN=2: a chain for every pair
  the product's plans   batch 1 (small-batch plan) and batch 3 (two-level launches + the chain for the last three levels)
Launches of few workgroups run 8 waves per workgroup, large ones (the benchmark's) 4: the threshold is read once per process (HS_PYRAMID_NW8), so the
4-wave instances of the same kernels run in a child process that executes this file as a script with HS_PYRAMID_NW8=0.
Shapes: 209 x 97 (one column past a 208-px level-B tile, a partial last tile row), 64 x 48 (a single tile, levels smaller than a tile), 417 x 33 (a row
count that leaves a one-row last tile), 641 x 97 (several tile columns of the two-level kernel, the last one partial).  Images: all 0, all 255 (a + b + 2 at its largest: 2 * 510 + 2), 0/255 checkerboards of 4-px and 1-px fields (both extremes and the
mixes of them side by side), seeded noise."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import hyslam_amd as HS

pytestmark = pytest.mark.gpu
SHAPES = ((209, 97), (64, 48), (417, 33), (641, 97))
LEVELS = 8
NFEAT = 500

PLANNED_AT = (209, 97)      # the shape at which the launch counts are asserted: a frame too narrow for the two-level kernel (its level-A region must fit over the
                            # source rectangle in LDS) is planned level by level whatever the knobs say, and still has to come out right
PATHS = {
    "level_lds": {"HS_PYRAMID_NO_FUSE": "1"},
    "two_levels": {"HS_PYRAMID_CHAIN": "0", "HS_PYRAMID_DEEP_MAX": "0"},
    "chain_pairs": {"HS_PYRAMID_CHAIN": "2", "HS_PYRAMID_DEEP_MAX": "0"},
    "product": {},
}


def images(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(1000 * w + h)
    return {"zeros": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8),
            "checker": ((((xx >> 2) + (yy >> 2)) & 1) * 255).astype(np.uint8), "checker1": (((xx + yy) & 1) * 255).astype(np.uint8),
            "noise": rng.integers(0, 256, (h, w), dtype=np.uint8)}


def make_reference():
    """{(w, h): (names, frames, [oracle pyramid per frame])}: computed once, shared by every path, never written to"""
    p = oracle.default_params(NFEAT, 1.2, LEVELS)
    ref = {}
    for w, h in SHAPES:
        im = images(w, h)
        pyr = []
        for f in im.values():
            lv = [f]
            for l in range(1, LEVELS):
                lv.append(oracle.resize_linear(lv[-1], *oracle.pyramid_size(p, w, h, l)))      # ComputePyramid: level l from level l - 1
            for a in lv:
                a.setflags(write=False)
            pyr.append(lv)
        ref[(w, h)] = (list(im.keys()), list(im.values()), pyr)
    return ref


@pytest.fixture(scope="module")
def reference():
    return make_reference()


def check_call(ex, names, frames, pyr, what):
    ex.extract_batch(frames)
    n = ex.pyramid_launches()
    for i, name in enumerate(names):
        for l in range(1, LEVELS):
            got = ex.debug_level(i, l)
            assert got.shape == pyr[i][l].shape, (what, name, l, got.shape, pyr[i][l].shape)
            bad = np.argwhere(got != pyr[i][l])
            assert len(bad) == 0, "%s, image %r, level %d: %d bytes differ, first at (row %d, col %d): device %d, oracle %d" % (
                what, name, l, len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], pyr[i][l][tuple(bad[0])])
    return n


def check_path(reference, shape, path):
    """the handle is created by the caller's environment (the knobs are read at creation)"""
    names, frames, pyr = reference[shape]
    ex = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=NFEAT, fScaleFactor=1.2, nLevels=LEVELS))
    what = "%dx%d, %s" % (shape + (path,))
    # one frame per call: the small-batch plan where it is on
    n1 = [check_call(ex, [nm], [f], [q], what + ", batch 1") for nm, f, q in zip(names, frames, pyr)]
    assert len(set(n1)) == 1, (what, n1)
    # three frames per call: the standard plan
    n3 = check_call(ex, names[:3], frames[:3], pyr[:3], what + ", batch 3")
    assert check_call(ex, names[2:], frames[2:], pyr[2:], what + ", batch 3 (other frames)") == n3
    print(what, "launches per call: batch 1", n1[0], "batch 3", n3)
    if path == "level_lds":
        assert n1[0] == LEVELS - 1 and n3 == LEVELS - 1, (what, n1, n3)           # a launch per level: nothing fused
    if shape != PLANNED_AT:
        return
    if path == "two_levels":
        assert n1[0] == n3 and (LEVELS - 1) // 2 + 1 <= n3 < LEVELS - 1, (what, n1, n3)   # no launch makes more than two levels, and some make two
    elif path == "chain_pairs":
        assert n1[0] == n3 and n3 <= (LEVELS - 1) // 2 + 1, (what, n1, n3)
    elif path == "product":
        assert n1[0] <= 2 and n3 < LEVELS - 1, (what, n1, n3)                     # batch 1: seven levels in two launches at most, so a chain of >= 4 ran


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_level_matches_the_oracle(gpu, monkeypatch, reference, shape, path):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    check_path(reference, shape, path)


def test_four_wave_workgroups_in_a_child_process(gpu):
    """every shape and path again with 4 waves per workgroup (k_resize_two_levels<4>, k_resize_chain<4>: what launches of many frames run)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    e["HS_PYRAMID_NW8"] = "0"
    e["PYTHONPATH"] = os.pathsep.join([root, os.path.join(root, "tests"), e.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PYRAMID_COMBINE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


if __name__ == "__main__":
    ref = make_reference()
    for shape in SHAPES:
        for path, env in PATHS.items():
            for k in ("HS_PYRAMID_NO_FUSE", "HS_PYRAMID_CHAIN", "HS_PYRAMID_DEEP_MAX"):
                os.environ.pop(k, None)
            os.environ.update(env)
            check_path(ref, shape, path)
    print("PYRAMID_COMBINE_OK", os.environ.get("HS_PYRAMID_NW8"))
