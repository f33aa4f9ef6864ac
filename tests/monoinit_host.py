"""The file formats of tests/cpp/monoinit_sanitize/monoinit_host_math (the kernels' math of kernels_monoinit.hip as a single-thread host program) and
the comparison of one result with the LITERAL reference of tests/ref_monoinit.py, shared by tests/test_monoinit_abi.py, the GPU tests and
tools/bench_monoinit.py."""
import struct

import numpy as np

PARAMS_FMT = "<5fiiffiQ"              # hs_monoinit_params, 48 bytes
RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_matches", "<i4"), ("model", "<i4"), ("best_solution", "<i4"), ("best_it_h", "<i4"), ("best_it_f", "<i4"),
                         ("n_triangulated", "<i4"), ("_pad", "<i4"), ("score_h", "<f4"), ("score_f", "<f4"), ("rh", "<f4"), ("cos_parallax", "<f4"),
                         ("H21", "<f4", 9), ("F21", "<f4", 9), ("n_good", "<i4", 8), ("R21", "<f4", 9), ("t21", "<f4", 3)])
RESULT_INTS = ("status", "n_matches", "model", "best_solution", "best_it_h", "best_it_f", "n_triangulated")
RESULT_FLOATS = ("score_h", "score_f", "rh", "cos_parallax", "H21", "F21", "R21", "t21")


def pack_params(p):
    return struct.pack(PARAMS_FMT, p["fx"], p["fy"], p["cx"], p["cy"], p["sigma"], p["max_iterations"], p["min_triangulated"], p["min_frac_triangulated"],
                       p["min_parallax_deg"], 0, p["seed"])


def write_problem(path, c):
    k1, k2 = np.ascontiguousarray(c["kps1"], np.float32), np.ascontiguousarray(c["kps2"], np.float32)
    draws = np.zeros((0, 8), np.uint32) if c["draws"] is None else np.ascontiguousarray(c["draws"], np.uint32)
    with open(path, "wb") as f:
        f.write(pack_params(c["params"]))
        f.write(struct.pack("<4i", len(k1), len(k2), len(draws), 0))
        f.write(k1.tobytes())
        f.write(k2.tobytes())
        f.write(np.ascontiguousarray(c["matches12"], np.int32).tobytes())
        f.write(draws.tobytes())


def read_output(path, n1):
    raw = open(path, "rb").read()
    N, H = struct.unpack_from("<2i", raw, 0)
    o = 8
    score = np.frombuffer(raw, np.float32, 2 * H, o).reshape(2, H)
    o += 8 * H
    model = np.frombuffer(raw, np.float32, 2 * H * 9, o).reshape(2, H, 9)
    o += 72 * H
    res = np.frombuffer(raw, RESULT_DTYPE, 1, o)[0]
    o += RESULT_DTYPE.itemsize
    inl_h, inl_f = np.frombuffer(raw, np.uint8, n1, o), np.frombuffer(raw, np.uint8, n1, o + n1)
    o += 2 * n1
    p3d = np.frombuffer(raw, np.float32, 3 * n1, o).reshape(n1, 3)
    tri = np.frombuffer(raw, np.uint8, n1, o + 12 * n1)
    assert o + 13 * n1 == len(raw)
    return dict(N=N, H=H, score=score, model=model, res=res, inliers_h=inl_h, inliers_f=inl_f, p3d=p3d, triangulated=tri)


def same(a, b):
    return np.array_equal(np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1), equal_nan=True)


def compare(tag, res, inl_h, inl_f, p3d, tri, ref):
    """one problem's outputs against the reference's dict, field by field; floats by value with NaN equal to NaN"""
    for k in RESULT_INTS:
        assert int(res[k]) == int(ref[k]), (tag, k, int(res[k]), int(ref[k]))
    assert np.array_equal(np.asarray(res["n_good"]), ref["n_good"]), (tag, "n_good", res["n_good"], ref["n_good"])
    for k in RESULT_FLOATS:
        assert same(res[k], ref[k]), (tag, k, res[k], ref[k])
    assert np.array_equal(inl_h, ref["inliers_h"]), (tag, "inliers_h", int((inl_h != ref["inliers_h"]).sum()))
    assert np.array_equal(inl_f, ref["inliers_f"]), (tag, "inliers_f", int((inl_f != ref["inliers_f"]).sum()))
    assert np.array_equal(tri, ref["triangulated"]), (tag, "triangulated")
    assert same(p3d, ref["p3d"]), (tag, "p3d")


def compare_hypotheses(tag, out, ref):
    """the host program's per-hypothesis scores and models against the reference's"""
    hyp = ref["hyp"]
    if hyp is None:
        return 0
    for m, (sk, mk) in enumerate((("score_h", "H21"), ("score_f", "F21"))):
        for it in range(out["H"]):
            assert same(out["model"][m, it], hyp[mk][it]), (tag, mk, it, out["model"][m, it], hyp[mk][it].reshape(-1))
            assert same(out["score"][m, it], hyp[sk][it]), (tag, sk, it, out["score"][m, it], hyp[sk][it])
    return 2 * out["H"]
