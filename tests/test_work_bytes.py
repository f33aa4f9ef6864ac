"""The caller-owned work areas (`d_work`) of the resident chain: sizes and layouts, without a GPU.

tests/golden/work_bytes.json holds every public hs_*_work_bytes over a grid, recorded by tools/record_work_bytes.py from the build BEFORE the layouts
moved into hyslam_amd/csrc/hs_work.h; the numbers are that build's, never the code under test's.  The sizes are pure host code, so the library
answers here as it does for tests/test_abi.py."""
import itertools
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
N = [-1, 0, 1, 31, 32, 33, 63, 64, 65, 2000, 65535]
L = [-1, 0, 1, 255, 256, 257, 1023, 1024, 1025, 50000]
KF_CAP = [0, 1, 63, 64, 65, 1000]
# the dimensions every function is recorded over (the grid above); the file may add values of arguments the sizes ignore
GRID = {"hs_track_work_bytes": {0: N, 2: L}, "hs_local_points_work_bytes": {0: L}, "hs_local_map_work_bytes": {0: L},
        "hs_keyframe_work_bytes": {0: N, 1: KF_CAP}, "hs_track_refkf_work_bytes": {0: N, 1: KF_CAP, 2: L}, "hs_pose_work_bytes": {}}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "work_bytes.json")) as f:
        g = json.load(f)
    assert (g["n"], g["L"], g["kf_cap"]) == (N, L, KF_CAP)
    assert sorted(g["sizes"]) == sorted(GRID)
    return g["sizes"]


def test_recorded_sizes_cover_the_grid(golden):
    for name, dims in GRID.items():
        rows = golden[name]
        assert len({tuple(r[:-1]) for r in rows}) == len(rows), name
        for pos, values in dims.items():
            assert {r[pos] for r in rows} == set(values), (name, pos)
        others = [sorted({r[p] for r in rows}) for p in range(len(rows[0]) - 1)]
        assert len(rows) == len(list(itertools.product(*others))), name          # the full product, no hole


def test_every_work_size_equals_the_recorded_one(golden):
    from hyslam_amd import _native as N_
    lib = N_.lib()
    for name, rows in golden.items():
        f = getattr(lib, name)
        for *args, want in rows:
            assert int(f(*args)) == want, (name, args, int(f(*args)), want)


def test_work_sizes_do_not_decrease_in_any_dimension(golden):
    from hyslam_amd import _native as N_
    lib = N_.lib()
    for name, rows in golden.items():
        f = getattr(lib, name)
        size = {tuple(r[:-1]): int(f(*r[:-1])) for r in rows}
        for pos in range(len(rows[0]) - 1):
            lines = {}                                            # the other arguments fixed, this one ascending
            for args in sorted(size):
                lines.setdefault(args[:pos] + args[pos + 1:], []).append(size[args])
            for rest, v in lines.items():
                assert v == sorted(v), (name, pos, rest, v)


def test_layout_structs_under_sanitizers(golden):
    """tests/cpp/test_work_layout.cpp over hyslam_amd/csrc/hs_work.h alone: a stand-alone host program under ASan + UBSan (nothing is loaded into python)"""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "test_work_layout")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_work_layout.cpp"), "-o", exe])
    text = "".join("%s %s\n" % (name, " ".join(str(v) for v in r)) for name, rows in golden.items() if name != "hs_pose_work_bytes" for r in rows)
    r = subprocess.run([exe], input=text.encode(), capture_output=True, timeout=120)
    assert r.returncode == 0 and b"WORK LAYOUT OK" in r.stdout, r.stdout + r.stderr
    assert b"%d recorded sizes" % text.count("\n") in r.stdout, r.stdout
