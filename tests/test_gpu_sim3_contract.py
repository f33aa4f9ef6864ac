"""GPU: the contract of hs_sim3_iterate(_device) beyond its values — the results do not depend on what the work area, the outputs and the handle's
scratch held beforehand; the device form does all of its work in the order of the caller's stream and synchronises nothing; a refused call touches no
output."""
import numpy as np
import pytest

import hipmem
import ref_sim3 as R
import sim3_cases as SC
import sim3_gpu as G

pytestmark = pytest.mark.gpu

NAMES = ["n30_same_camera", "n100_rounds", "too_few", "equal_counts_last_wins", "identical_sets", "n257"]


@pytest.fixture(scope="module")
def ex(gpu):
    import hyslam_amd as HS
    return HS.ORBExtractor(device=0)


def test_results_do_not_depend_on_earlier_contents(ex):
    """host form == device form == the same call again == the device form over another fill of its work area and outputs == the host form behind
    hs_debug_poison, byte for byte, over a batch with a second call"""
    from hyslam_amd import _native as N
    cases = [SC.cases()[n] for n in NAMES]

    def both_calls(runner):
        states, best = G.fresh(cases)
        out = []
        for n_it in (7, 5):
            res, inl = runner(ex, cases, n_it, states, best)
            out.append((res.tobytes(), inl.tobytes(), states.tobytes(), best.tobytes()))
        return out

    host = both_calls(G.run_host)
    stream = hipmem.Stream(non_blocking=True)
    assert both_calls(lambda *a: G.run_device(*a, stream)) == host, "device form differs from host form"
    assert both_calls(lambda *a: G.run_device(*a, stream, fill=0xA7)) == host, "the result depends on what the work area or the outputs held"
    assert both_calls(G.run_host) == host, "the same call twice differs"
    try:
        assert ex._lib.hs_debug_poison(0xA7) == N.HS_OK
        assert both_calls(G.run_host) == host, "the result depends on what the scratch held"
        assert ex._lib.hs_debug_poison(0x00) == N.HS_OK
        assert both_calls(G.run_host) == host, "the result depends on what the scratch held"
    finally:
        ex._lib.hs_debug_poison(-1)


def test_device_form_behind_a_pending_write_of_its_inputs(ex):
    """the device form on a caller's stream: the real inputs arrive behind a delay on that stream, the outputs are snapshotted right behind the call"""
    import stream_order as SO
    from hyslam_amd import _native as N
    real = SC.cases()["n30_same_camera"]
    decoy = dict(real, corrs=SC.scene(77, 30))                     # another valid problem of the same size under the call's parameters
    n, n_it = 30, 12
    par, off, corrs_r, _, _ = G.pack([real])
    _, _, corrs_d, _, _ = G.pack([decoy])
    exp, dexp = SC.solver(real).iterate(n_it), SC.solver(decoy).iterate(n_it)
    assert exp["status"] == R.FOUND and not np.array_equal(exp["mask"], dexp["mask"])
    st0, _ = G.fresh([real])
    nwork = ex._lib.hs_sim3_work_bytes(1, n, G.bound([real], n_it))

    def scene():
        def call(ptr, stream):
            N.check(ex._h, ex._lib.hs_sim3_iterate_device(ex._h, 1, G.p(par), G.p(off), ptr["corrs"], n_it, None, 0, ptr["states"], ptr["best"], ptr["results"], ptr["inl"],
                                                          ptr["work"], stream))
        return [SO.Step("sim3_iterate", dict(corrs=(corrs_r, corrs_d), states=(st0, st0.copy())), dict(results=N.SIM3_RESULT_DTYPE.itemsize, inl=n, best=n), call,
                        dict(inl=[(0, exp["mask"], dexp["mask"])]), work=dict(work=nwork))]

    for steps, got, after in SO.run(ex, scene, tag="hs_sim3_iterate_device"):
        SO.check(steps, got, after, "hs_sim3_iterate_device")
        res = got[0]["results"].view(N.SIM3_RESULT_DTYPE)[0]
        assert int(res["status"]) == R.FOUND and G.same(res["T12"], exp["T12"]) and int(res["n_inliers"]) == exp["n_inliers"]


def test_refused_calls_leave_the_outputs_alone(ex):
    """with a real handle: every refusal is HS_ERR_INVALID before anything is enqueued, and no output byte changes, in both forms"""
    from hyslam_amd import _native as N
    c = SC.cases()["n30_same_camera"]
    par, off, corrs, _, _ = G.pack([c])
    states, best = G.fresh([c])
    inl, res = np.full(len(corrs), G.FILL, np.uint8), np.full(N.SIM3_RESULT_DTYPE.itemsize, G.FILL, np.uint8)
    p = G.p
    neg_min = par.copy()
    neg_min["min_inliers"] = -1
    bad_off = np.array([-1, 30], np.int64)
    big = np.array([0, 1 << 31], np.int64)                         # a problem of 2^31 correspondences: refused before anything is read
    for args in ((0, par, off, corrs, 5), (1, par, off, corrs, 0), (1, par, off, corrs, -1), (1, neg_min, off, corrs, 5), (1, par, off[::-1].copy(), corrs, 5),
                 (1, par, bad_off, corrs, 5), (1, par, big, corrs, 5), (1, None, off, corrs, 5), (1, par, None, corrs, 5), (1, par, off, None, 5)):
        Q, pp, po, pc, n = args
        st = ex._lib.hs_sim3_iterate(ex._h, Q, p(pp) if pp is not None else None, p(po) if po is not None else None, p(pc) if pc is not None else None, n, None, 0,
                                     p(states), p(best), p(res), p(inl))
        assert st == N.HS_ERR_INVALID, args[0:1] + args[4:]
    assert ex._lib.hs_sim3_iterate(ex._h, 1, p(par), p(off), p(corrs), 5, None, 1, p(states), p(best), p(res), p(inl)) == N.HS_ERR_INVALID, "draw_cap without a table"
    assert ex._lib.hs_sim3_iterate(ex._h, 1, p(par), p(off), p(corrs), 5, None, 0, None, p(best), p(res), p(inl)) == N.HS_ERR_INVALID
    assert ex._lib.hs_sim3_iterate(ex._h, 1, p(par), p(off), p(corrs), 5, None, 0, p(states), None, p(res), p(inl)) == N.HS_ERR_INVALID
    assert ex._lib.hs_sim3_iterate(ex._h, 1, p(par), p(off), p(corrs), 5, None, 0, p(states), p(best), None, p(inl)) == N.HS_ERR_INVALID
    assert ex._lib.hs_sim3_iterate(ex._h, 1, p(par), p(off), p(corrs), 5, None, 0, p(states), p(best), p(res), None) == N.HS_ERR_INVALID
    for field in ("iterations", "best_inliers"):
        neg = states.copy()
        neg[field] = -1
        assert ex._lib.hs_sim3_iterate(ex._h, 1, p(par), p(off), p(corrs), 5, None, 0, p(neg), p(best), p(res), p(inl)) == N.HS_ERR_INVALID, "a state with a negative count"
    assert (inl == G.FILL).all() and (res == G.FILL).all() and (best == G.FILL).all() and not states.view(np.uint8).any()
    # the device form: the same predicate, and a missing or misaligned work area or misaligned correspondences
    d_corrs, d_states, d_best = hipmem.DevBuf.from_numpy(corrs), G.guarded(states), G.guarded(best)
    d_res, d_inl = G.out_buf(N.SIM3_RESULT_DTYPE.itemsize), G.out_buf(len(corrs))
    nwork = ex._lib.hs_sim3_work_bytes(1, len(corrs), 5)
    d_work = G.out_buf(nwork)
    dev = lambda Q, pp, po, pc, n, work: ex._lib.hs_sim3_iterate_device(ex._h, Q, p(pp), p(po), pc, n, None, 0, d_states.ptr, d_best.ptr, d_res.ptr, d_inl.ptr, work, None)
    for args in ((0, par, off, d_corrs.ptr, 5, d_work.ptr), (1, par, off, d_corrs.ptr, 0, d_work.ptr), (1, neg_min, off, d_corrs.ptr, 5, d_work.ptr),
                 (1, par, bad_off, d_corrs.ptr, 5, d_work.ptr), (1, par, big, d_corrs.ptr, 5, d_work.ptr), (1, par, off, d_corrs.ptr + 8, 5, d_work.ptr),
                 (1, par, off, d_corrs.ptr, 5, None), (1, par, off, d_corrs.ptr, 5, d_work.ptr + 8)):
        assert dev(*args) == N.HS_ERR_INVALID, args[0:1] + args[4:5]
    hipmem.sync()
    assert (G.read(d_res, np.uint8, N.SIM3_RESULT_DTYPE.itemsize) == G.FILL).all() and (G.read(d_inl, np.uint8, len(corrs)) == G.FILL).all()
    assert (G.read(d_best, np.uint8, len(corrs)) == G.FILL).all() and not G.read(d_states, np.uint8, states.nbytes).any() and (G.read(d_work, np.uint8, nwork) == G.FILL).all()
    assert dev(1, par, off, d_corrs.ptr, 5, d_work.ptr) == N.HS_OK                                   # and the call they refused is a valid one
    hipmem.sync()
    assert G.read(d_res, N.SIM3_RESULT_DTYPE, 1)["status"][0] == SC.solver(c).iterate(5)["status"]
