#!/usr/bin/env python3
"""Records every public hs_*_work_bytes of ONE build of the library into tests/golden/work_bytes.json.

    make -C hyslam_amd/csrc BUILD=<dir> OUT=<dir>/libhyslam_amd.so        (at the commit whose sizes are the reference)
    python tools/record_work_bytes.py <dir>/libhyslam_amd.so

The sizes are pure host code, so no GPU is needed.  tests/test_work_bytes.py compares the working tree's library with the file: the numbers in it must
come from the commit a layout change is measured against, never from the code under test.  Each row is [arguments..., bytes]."""
import ctypes as C
import itertools
import json
import os
import sys

N = [-1, 0, 1, 31, 32, 33, 63, 64, 65, 2000, 65535]            # keypoints of a frame
L = [-1, 0, 1, 255, 256, 257, 1023, 1024, 1025, 50000]         # landmarks of the map
KF_CAP = [0, 1, 63, 64, 65, 1000]
# name -> (ctypes argument types, one list of values per argument); sizes the library ignores today get two values, so that a change shows
FUNCTIONS = {
    "hs_track_work_bytes": ([C.c_int] * 4, [N, [0, 2000], L, [0, 1000]]),                 # n, n_last, L, cap
    "hs_local_points_work_bytes": ([C.c_int], [L]),
    "hs_local_map_work_bytes": ([C.c_int], [L]),
    "hs_keyframe_work_bytes": ([C.c_int] * 3, [N, KF_CAP, [0, 100]]),                     # n, kf_cap, new_cap
    "hs_track_refkf_work_bytes": ([C.c_int] * 3, [N, KF_CAP, L]),                         # n, kf_cap, L
    "hs_pose_work_bytes": ([C.c_int, C.c_int64], [[0, 1, 64], [0, 1, 65535, 1 << 33]]),   # Q, n_edges_total
}


def record(lib_path):
    lib = C.CDLL(lib_path)
    sizes = {}
    for name, (argtypes, values) in FUNCTIONS.items():
        f = getattr(lib, name)
        f.argtypes, f.restype = argtypes, C.c_size_t
        sizes[name] = [list(a) + [int(f(*a))] for a in itertools.product(*values)]
    return sizes


if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "work_bytes.json")
    with open(out, "w") as fh:
        json.dump({"n": N, "L": L, "kf_cap": KF_CAP, "sizes": record(sys.argv[1])}, fh, separators=(",", ":"))
        fh.write("\n")
    print("wrote", out)
