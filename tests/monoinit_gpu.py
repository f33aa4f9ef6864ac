"""What tests/test_gpu_monoinit.py and tests/test_gpu_monoinit_contract.py share: packing the cases of tests/monoinit_cases.py into one call of
hs_monoinit_estimate(_device), running the host and the device form on sentinel-filled, guarded outputs, and comparing every problem of the call
with the LITERAL reference of tests/ref_monoinit.py field by field (tests/monoinit_host.py: floats by value with NaN equal to NaN)."""
import ctypes as C
import functools

import numpy as np

import hipmem
import monoinit_cases as MC
import monoinit_host as MH
import ref_monoinit as R

GUARD = 64
FILL = 0x55


def p(a):
    return a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def reference(name):
    """LITERAL of a named case or sweep scene, computed once and shared"""
    c = MC.cases().get(name) or MC.sweep()[name]
    return MC.run_reference(c)


def pack(cases):
    """params [Q], off1, off2 [Q + 1], kps1, kps2 (KP_DTYPE), matches12, draws [Q, cap, 8] or None, cap.  A table shorter than the call's cap is
    continued with the generator's own words, which is what draw_cap <= it means for that problem."""
    import ref_pnp
    from hyslam_amd import _native as N
    Q = len(cases)
    par = np.zeros(Q, N.MONOINIT_PARAMS_DTYPE)
    for q, c in enumerate(cases):
        for k in ("fx", "fy", "cx", "cy", "sigma", "max_iterations", "min_triangulated", "min_frac_triangulated", "min_parallax_deg", "seed"):
            par[k][q] = c["params"][k]
    off1, off2 = np.zeros(Q + 1, np.int64), np.zeros(Q + 1, np.int64)
    off1[1:], off2[1:] = np.cumsum([len(c["kps1"]) for c in cases]), np.cumsum([len(c["kps2"]) for c in cases])

    def kp(xy):
        k = np.zeros(len(xy), N.KP_DTYPE)
        k["x"], k["y"], k["size"], k["octave"] = xy[:, 0], xy[:, 1], 31.0, 0
        return k
    kps1, kps2 = np.concatenate([kp(c["kps1"]) for c in cases]), np.concatenate([kp(c["kps2"]) for c in cases])
    matches = np.concatenate([np.asarray(c["matches12"], np.int32) for c in cases])
    cap = max([0] + [len(c["draws"]) for c in cases if c["draws"] is not None])
    draws = None
    if cap:
        draws = np.zeros((Q, cap, R.DRAW_STRIDE), np.uint32)
        for q, c in enumerate(cases):
            for it in range(cap):
                draws[q, it] = [ref_pnp.draw32(c["params"]["seed"], it, k, 8, c["draws"]) for k in range(8)]
    return par, off1, off2, kps1, kps2, matches, draws, cap


def bound(cases):
    return max(c["params"]["max_iterations"] for c in cases)


def run_host(ex, cases):
    """the C ABI host form on sentinel-filled outputs with guards -> (results, inliers_h, inliers_f, p3d, triangulated)"""
    from hyslam_amd import _native as N
    par, off1, off2, kps1, kps2, matches, draws, cap = pack(cases)
    Q, n1, rb = len(cases), len(kps1), N.MONOINIT_RESULT_DTYPE.itemsize
    res = np.full(Q * rb + GUARD, FILL, np.uint8)
    ih, jf, tri = (np.full(n1 + GUARD, FILL, np.uint8) for _ in range(3))
    p3d = np.full(12 * n1 + GUARD, FILL, np.uint8)
    N.check(ex._h, ex._lib.hs_monoinit_estimate(ex._h, Q, p(par), p(off1), p(kps1), p(off2), p(kps2), p(matches), p(draws) if cap else None, cap, p(res), p(ih), p(jf),
                                                p(p3d), p(tri)))
    for a, n in ((res, Q * rb), (ih, n1), (jf, n1), (tri, n1), (p3d, 12 * n1)):
        assert (a[n:] == FILL).all(), "bytes written behind an output"
    return (res[:Q * rb].view(N.MONOINIT_RESULT_DTYPE).copy(), ih[:n1].copy(), jf[:n1].copy(), p3d[:12 * n1].view(np.float32).reshape(n1, 3).copy(), tri[:n1].copy())


def out_buf(nbytes, fill=FILL):
    b = hipmem.DevBuf(nbytes + GUARD)
    b.fill(fill)
    return b


def read(buf, dtype, count, fill=FILL):
    nbytes = np.dtype(dtype).itemsize * count
    raw = buf.to_numpy(np.uint8, nbytes + GUARD)
    assert (raw[nbytes:] == fill).all(), "bytes written behind the output"
    return raw[:nbytes].view(dtype).copy()


def run_device(ex, cases, stream, fill=FILL):
    """the device form on a caller's stream; the work area is the size hs_monoinit_work_bytes gives for the call's bound, filled and guarded too"""
    from hyslam_amd import _native as N
    par, off1, off2, kps1, kps2, matches, draws, cap = pack(cases)
    Q, n1 = len(cases), len(kps1)
    nwork = ex._lib.hs_monoinit_work_bytes(Q, n1, bound(cases))
    d_k1, d_k2, d_m = hipmem.DevBuf.from_numpy(kps1), hipmem.DevBuf.from_numpy(kps2), hipmem.DevBuf.from_numpy(matches)
    d_draws = hipmem.DevBuf.from_numpy(draws) if cap else None
    d_res, d_ih, d_if = out_buf(Q * N.MONOINIT_RESULT_DTYPE.itemsize, fill), out_buf(n1, fill), out_buf(n1, fill)
    d_p3d, d_tri, d_work = out_buf(12 * n1, fill), out_buf(n1, fill), out_buf(nwork, fill)
    N.check(ex._h, ex._lib.hs_monoinit_estimate_device(ex._h, Q, p(par), p(off1), d_k1.ptr, p(off2), d_k2.ptr, d_m.ptr, d_draws.ptr if cap else None, cap, d_res.ptr,
                                                       d_ih.ptr, d_if.ptr, d_p3d.ptr, d_tri.ptr, d_work.ptr, stream.ptr))
    stream.synchronize()
    read(d_work, np.uint8, nwork, fill)
    return (read(d_res, N.MONOINIT_RESULT_DTYPE, Q, fill), read(d_ih, np.uint8, n1, fill), read(d_if, np.uint8, n1, fill),
            read(d_p3d, np.float32, 3 * n1, fill).reshape(n1, 3), read(d_tri, np.uint8, n1, fill))


def compare_call(tag, cases, refs, out):
    res, ih, jf, p3d, tri = out
    off = np.concatenate([[0], np.cumsum([len(c["kps1"]) for c in cases])]).astype(np.int64)
    for q, ref in enumerate(refs):
        sl = slice(off[q], off[q + 1])
        MH.compare("%s problem %d" % (tag, q), res[q], ih[sl], jf[sl], p3d[sl], tri[sl], ref)
