"""What tests/test_gpu_sim3.py and tests/test_gpu_sim3_contract.py share: packing the cases of tests/sim3_cases.py into one call of
hs_sim3_iterate(_device), running the host and the device form on sentinel-filled, guarded outputs, and comparing one problem of one call with the
D19 reference of tests/ref_sim3.py field by field (floats by value with NaN equal to NaN: the payload of a NaN is not part of the definition)."""
import ctypes as C

import numpy as np

import hipmem
import ref_sim3 as R

GUARD = 64
FILL = 0x55


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def pack(cases):
    """params [Q], offsets [Q + 1], corrs, draws [Q, cap, DRAW_STRIDE] or None, cap.  A table shorter than the call's cap is continued with the
    generator's own words, which is what draw_cap <= it means for that problem."""
    from hyslam_amd import _native as N
    Q = len(cases)
    par = np.zeros(Q, N.SIM3_PARAMS_DTYPE)
    for q, c in enumerate(cases):
        for k in ("probability", "min_inliers", "max_iterations", "fix_scale", "seed"):
            par[k][q] = c["params"][k]
        par["fx1"][q], par["fy1"][q], par["cx1"][q], par["cy1"][q] = c["k1"]
        par["fx2"][q], par["fy2"][q], par["cx2"][q], par["cy2"][q] = c["k2"]
    off = np.zeros(Q + 1, np.int64)
    off[1:] = np.cumsum([len(c["corrs"]) for c in cases])
    corrs = np.concatenate([np.ascontiguousarray(c["corrs"]).view(N.SIM3_CORR_DTYPE) for c in cases])
    cap = max([0] + [len(c["draws"]) for c in cases if c["draws"] is not None])
    draws = None
    if cap:
        draws = np.zeros((Q, cap, R.DRAW_STRIDE), np.uint32)
        for q, c in enumerate(cases):
            for it in range(cap):
                draws[q, it, :3] = [R.draw32(c["params"]["seed"], it, k, c["draws"]) for k in range(3)]
    return par, off, corrs, draws, cap


def fresh(cases):
    from hyslam_amd import _native as N
    return np.zeros(len(cases), N.SIM3_STATE_DTYPE), np.full(sum(len(c["corrs"]) for c in cases), FILL, np.uint8)


def bound(cases, n_iterations):
    return max(1, max(min(n_iterations, R.plan(len(c["corrs"]), **c["params"])[0]) for c in cases))


def run_host(ex, cases, n_iterations, states, best):
    """the C ABI host form on sentinel-filled outputs with guards -> (results, inlier masks); states and best are updated in place"""
    from hyslam_amd import _native as N
    par, off, corrs, draws, cap = pack(cases)
    Q, n, rb = len(cases), len(corrs), N.SIM3_RESULT_DTYPE.itemsize
    inl = np.full(n + GUARD, FILL, np.uint8)
    res = np.full(Q * rb + GUARD, FILL, np.uint8)
    N.check(ex._h, ex._lib.hs_sim3_iterate(ex._h, Q, p(par), p(off), p(corrs), n_iterations, p(draws) if cap else None, cap, p(states), p(best), p(res), p(inl)))
    assert (inl[n:] == FILL).all() and (res[Q * rb:] == FILL).all(), "bytes written behind the output"
    return res[:Q * rb].view(N.SIM3_RESULT_DTYPE).copy(), inl[:n].copy()


def out_buf(nbytes, fill=FILL):
    b = hipmem.DevBuf(nbytes + GUARD)
    b.fill(fill)
    return b


def guarded(a):
    a = np.ascontiguousarray(a)
    b = out_buf(a.nbytes)
    if a.nbytes:
        hipmem._ok(hipmem.hip().hipMemcpy(b.ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")
    return b


def read(buf, dtype, count, fill=FILL):
    nbytes = np.dtype(dtype).itemsize * count
    raw = buf.to_numpy(np.uint8, nbytes + GUARD)
    assert (raw[nbytes:] == fill).all(), "bytes written behind the output"
    return raw[:nbytes].view(dtype).copy()


def run_device(ex, cases, n_iterations, states, best, stream, fill=FILL):
    """the device form on a caller's stream; the work area is the size hs_sim3_work_bytes gives for the call's bound, filled and guarded too"""
    from hyslam_amd import _native as N
    par, off, corrs, draws, cap = pack(cases)
    Q, n = len(cases), len(corrs)
    nwork = ex._lib.hs_sim3_work_bytes(Q, n, bound(cases, n_iterations))
    d_corrs, d_draws = hipmem.DevBuf.from_numpy(corrs), (hipmem.DevBuf.from_numpy(draws) if cap else None)
    d_states, d_best = guarded(states), guarded(best)
    d_res, d_inl, d_work = out_buf(Q * N.SIM3_RESULT_DTYPE.itemsize, fill), out_buf(n, fill), out_buf(nwork, fill)
    N.check(ex._h, ex._lib.hs_sim3_iterate_device(ex._h, Q, p(par), p(off), d_corrs.ptr, n_iterations, d_draws.ptr if cap else None, cap, d_states.ptr, d_best.ptr,
                                                  d_res.ptr, d_inl.ptr, d_work.ptr, stream.ptr))
    stream.synchronize()
    read(d_work, np.uint8, nwork, fill)
    states[:] = read(d_states, N.SIM3_STATE_DTYPE, Q)
    best[:] = read(d_best, np.uint8, n)
    return read(d_res, N.SIM3_RESULT_DTYPE, Q, fill), read(d_inl, np.uint8, n, fill)


def same(a, b):
    return np.array_equal(np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1), equal_nan=True)


def compare(tag, res, state, best, inl, r, solver, state_before, best_before):
    """one problem of one call against the reference's result `r` and its solver after the call"""
    got = (int(res["status"]), int(res["n_inliers"]), int(res["at_iteration"]), int(res["iterations"]), int(res["hypotheses_run"]))
    want = (r["status"], r["n_inliers"], r["at_iteration"], r["iterations"], r["hypotheses_run"])
    assert got == want, (tag, "status, n_inliers, at_iteration, iterations, hypotheses_run", got, want)
    assert np.array_equal(inl, r["mask"]), (tag, "inlier mask", int((inl != r["mask"]).sum()))
    for k in ("T12", "R", "t", "s"):
        assert same(res[k], r[k]), (tag, k, res[k], r[k])
    if r["status"] == R.TOO_FEW:
        assert state.tobytes() == state_before.tobytes() and np.array_equal(best, best_before), (tag, "TOO_FEW touched the state")
        return
    assert (int(state["iterations"]), int(state["best_inliers"])) == (solver.iterations, solver.best_inliers), (tag, "state")
    if solver.best is None:
        assert state[["R", "t", "s", "T12"]].tobytes() == state_before[["R", "t", "s", "T12"]].tobytes() and np.array_equal(best, best_before), (tag, "no best, yet the state moved")
    else:
        assert np.array_equal(best, solver.best_mask), (tag, "best mask")
        for k, v in zip(("R", "t", "s", "T12"), solver.best):
            assert same(state[k], v), (tag, "state " + k)


def run_cases(ex, cases, runner, calls, tag=""):
    """every call of `calls` over the cases in one batch, each compared with the reference -> per call (results, inlier masks, states, best masks)"""
    off = np.concatenate([[0], np.cumsum([len(c["corrs"]) for c in cases])]).astype(np.int64)
    solvers = [R.Solver(c["corrs"], c["k1"], c["k2"], c["params"], c["draws"]) for c in cases]
    states, best = fresh(cases)
    out = []
    for k, n_it in enumerate(calls):
        before, best_before = states.copy(), best.copy()
        res, inl = runner(ex, cases, n_it, states, best)
        for q, (c, s) in enumerate(zip(cases, solvers)):
            r = s.iterate(n_it)
            sl = slice(off[q], off[q + 1])
            compare("%s problem %d call %d" % (tag, q, k), res[q], states[q], best[sl], inl[sl], r, s, before[q], best_before[sl])
        out.append((res.copy(), inl.copy(), states.copy(), best.copy()))
    return out
