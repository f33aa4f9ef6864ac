"""CPU: which levels the plan gives to the quadtree kernel's four-wave level instance (hs_quadtree_small_level / hs_quadtree_small_from, hs_plan.hip).

tests/cpp/test_quadtree_small_plan.cpp is compiled host-only together with the plan's sources (pure host code: no HIP call, no GPU) and prints one
figure per line.  The expected values are the limits the instance's LDS arrays set (HS_QT_LEVEL_* in hs_plan.h): 512 list entries for quota + 8,
2048 / 1024 bytes for the key tables of qt_w + 1 columns / qt_h + 1 rows, 256 tile counters, and a histogram pyramid of 2736 entries, which holds
depth 5 for up to 2 roots (2 * 1365) and depth 4 for up to 8 (8 * 341); a level of 9 roots has no key tables.  For 1920 x 1080 at 2000 features
@1.2 every quota fits (level 0: 434) and the tiles decide: level 1 is 1600 x 900 = 25 x 15 = 375 tiles, level 2 is 1333 x 750 = 21 x 12 = 252, so
k = 2.  At 9000 features @1.4 the quotas are 2758, 1970, 1407, 1005, 718, 513, 366, ...: level 5 misses by one entry (513 + 8), k = 6."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hyslam_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc is needed to compile the plan's host code")
    exe = str(tmp_path_factory.mktemp("qt_plan") / "test_quadtree_small_plan")
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_quadtree_small_plan.cpp")] + [os.path.join(CSRC, f) for f in ("hs_plan.hip", "hs_plan_pyramid.hip", "hs_plan_fast.hip")]
                          + ["-o", exe], timeout=600)
    out = {}
    for line in subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines():
        k, v = line.split(None, 1)
        out.setdefault(k, []).append(v)
    assert "error" not in out, out.get("error")
    return out


def one(figures, key):
    assert len(figures[key]) == 1
    return int(figures[key][0])


def test_list_capacity(figures):
    assert one(figures, "quota504") == 1 and one(figures, "quota505") == 0


def test_key_table_extents(figures):
    assert one(figures, "xtab2048") == 1 and one(figures, "xtab2049") == 0
    assert one(figures, "ytab1024") == 1 and one(figures, "ytab1025") == 0


def test_tile_counters(figures):
    assert one(figures, "tiles256") == 1 and one(figures, "tiles272") == 0
    assert one(figures, "tiles256x1") == 1 and one(figures, "tiles257x1") == 0


def test_roots_and_pyramid_depth(figures):
    assert [one(figures, "nini%d" % n) for n in (1, 2, 3, 8)] == [1, 1, 1, 1]
    assert one(figures, "nini9") == 0
    assert one(figures, "nini0") == 1                      # a level without a FAST cell: its workgroup has nothing to do


def test_first_level_of_the_configurations(figures):
    assert figures["quota0"] == ["434", "2758", "2758", "195"]
    assert one(figures, "k_1080p_2000") == 2 and one(figures, "ok_1080p_2000") == 0b11111100
    assert one(figures, "k_1080p_9000") == 6 and one(figures, "ok_1080p_9000") == 0b11000000      # never level 0: its list needs 2766 entries
    assert one(figures, "k_imaging_9000") == 6 and one(figures, "ok_imaging_9000") == 0b11000000
    assert one(figures, "k_416_900") == 0 and one(figures, "ok_416_900") == 0b11111111


def test_the_digest_does_not_move(figures):
    assert figures["digest_unchanged"] == ["1", "1", "1", "1"]
