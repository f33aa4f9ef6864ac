"""Initial pose estimation as one resident call (include/hyslam_amd.h: hs_track_reference_keyframe_device, hs_track_initial_device,
hs_track_normal_device), what can be checked without a GPU: the result record's layout against tests/ref_refkf.py, the work area's size against its
parts over the grid of tests/test_work_bytes.py, the calls' answer to a NULL handle, and HsInitialWork's carve under ASan + UBSan as a stand-alone
program (tests/cpp/test_work_layout_initial.cpp; nothing is loaded into python)."""
import ctypes as C
import itertools
import os
import subprocess

import ref_refkf as RR
from test_work_bytes import BUILD, KF_CAP, L, N, ROOT


def test_result_record_is_the_reference_dtype():
    from hyslam_amd import _native as N_
    assert N_.TRACK_INITIAL_RESULT_DTYPE.itemsize == 32 == RR.INIT_RESULT_DTYPE.itemsize
    assert N_.TRACK_INITIAL_RESULT_DTYPE.names == RR.INIT_RESULT_DTYPE.names
    for k in RR.INIT_RESULT_DTYPE.names:
        assert N_.TRACK_INITIAL_RESULT_DTYPE.fields[k][:2] == RR.INIT_RESULT_DTYPE.fields[k][:2], k
    assert (N_.HS_REFKF_OK, N_.HS_REFKF_BOW_FAILED, N_.HS_REFKF_SKIPPED) == (RR.REFKF_OK, RR.REFKF_BOW_FAILED, RR.REFKF_SKIPPED)
    assert C.sizeof(N_.TrackRefkfParams) == 16 and C.sizeof(N_.TrackInitialOut) == 15 * C.sizeof(C.c_void_p)
    # the header's text says the same: five int32 fields in this order and three words of padding
    text = open(os.path.join(ROOT, "include", "hyslam_amd.h")).read()
    body = text[text.index("typedef struct hs_track_initial_result {"):text.index("} hs_track_initial_result;")]
    at = [body.index("int32_t " + k) for k in ("refkf_status", "n_bow", "n_matches_map_refkf", "n_init", "success", "_pad[3]")]
    assert at == sorted(at) and body.count("int32_t") == 6


def test_work_bytes_hold_their_parts_and_never_decrease():
    from hyslam_amd import _native as N_
    lib = N_.lib()
    size = {}
    for n, l, k in itertools.product(N, L, KF_CAP):
        size[n, l, k] = got = int(lib.hs_track_initial_work_bytes(n, 64, l, 100, k))
        assert got >= int(lib.hs_track_work_bytes(n, 64, l, 100)) + int(lib.hs_track_refkf_work_bytes(n, 0, l)) + 8 * max(n, 0), (n, l, k, got)
        assert got == int(lib.hs_track_initial_work_bytes(n, 0, l, 0, k))               # n_last and cap: read by no layout today
    for pos in range(3):
        lines = {}                                                # the other arguments fixed, this one ascending
        for args in sorted(size):
            lines.setdefault(args[:pos] + args[pos + 1:], []).append(size[args])
        for rest, v in lines.items():
            assert v == sorted(v), (pos, rest, v)
    for n_last, cap in ((0, 0), (1, 1), (64, 100), (65535, 50000)):                      # ... and in the two arguments the grid does not vary
        assert int(lib.hs_track_initial_work_bytes(2000, n_last, 50000, cap, 300)) == size[2000, 50000, 0]


def test_a_null_handle_is_refused():
    from hyslam_amd import _native as N_
    lib = N_.lib()
    assert lib.hs_track_reference_keyframe_device(*[None] * 5, 80, *[None] * 11) == N_.HS_ERR_INVALID
    assert lib.hs_track_initial_device(None, None, 1, None, None, None, 64, None, None, None, 80, *[None] * 11) == N_.HS_ERR_INVALID
    assert lib.hs_track_normal_device(None, None, 0, None, None, None, 64, None, None, None, 80, *[None] * 5, 10, None, 100, *[None] * 7) == N_.HS_ERR_INVALID


def test_initial_layout_under_sanitizers():
    """tests/cpp/test_work_layout_initial.cpp over hyslam_amd/csrc/hs_work.h alone: carved over a malloc of exactly bytes(), every sub-array written end
    to end, no two overlapping, none past the end"""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "test_work_layout_initial")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_work_layout_initial.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, timeout=120)
    assert r.returncode == 0 and b"INITIAL WORK LAYOUT OK" in r.stdout, r.stdout + r.stderr
