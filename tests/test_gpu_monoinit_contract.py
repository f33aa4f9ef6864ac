"""GPU: the contract of hs_monoinit_estimate(_device) beyond its values — the results do not depend on what the work area, the outputs and the
handle's scratch held beforehand; the device form does all of its work in the order of the caller's stream and synchronises nothing; a refused call
touches no output; the alignment rules of the device form are enforced."""
import numpy as np
import pytest

import hipmem
import monoinit_cases as MC
import monoinit_gpu as G
import ref_monoinit as R

pytestmark = pytest.mark.gpu

NAMES = ["general_f", "n7_too_few", "plane_h", "both_scores_zero", "identical_points", "directed_draws", "chi_chunk+1"]


@pytest.fixture(scope="module")
def ex(gpu):
    import hyslam_amd as HS
    return HS.ORBExtractor(device=0)


def test_results_do_not_depend_on_earlier_contents(ex):
    """host form == device form == the same call again == the device form over another fill of its work area and outputs == the host form behind
    hs_debug_poison, byte for byte.  The batch holds a TOO_FEW problem, one without a model and one with NaN scores: every output is written always."""
    from hyslam_amd import _native as N
    cases = [MC.cases()[n] for n in NAMES]
    run = lambda runner: [a.tobytes() for a in runner(ex, cases)]
    host = run(G.run_host)
    G.compare_call("contract", cases, [G.reference(n) for n in NAMES], G.run_host(ex, cases))
    stream = hipmem.Stream(non_blocking=True)
    assert run(lambda *a: G.run_device(*a, stream)) == host, "device form differs from host form"
    assert run(lambda *a: G.run_device(*a, stream, fill=0xA7)) == host, "the result depends on what the work area or the outputs held"
    assert run(lambda *a: G.run_device(*a, stream, fill=0xFF)) == host, "the result depends on what the work area or the outputs held"
    try:
        assert ex._lib.hs_debug_poison(0xA7) == N.HS_OK
        assert run(G.run_host) == host, "the result depends on what the scratch held"
        assert ex._lib.hs_debug_poison(0x00) == N.HS_OK
        assert run(G.run_host) == host, "the result depends on what the scratch held"
    finally:
        ex._lib.hs_debug_poison(-1)


def test_device_form_behind_a_pending_write_of_its_inputs(ex):
    """the device form on a caller's stream: the real inputs arrive behind a delay on that stream, the outputs are snapshotted right behind the call"""
    import stream_order as SO
    from hyslam_amd import _native as N
    real = MC.cases()["min_tri_below_accepted"]
    decoy = dict(real, matches12=np.roll(real["matches12"], 1))   # the same frames matched otherwise: another valid problem of the same size
    par, off1, off2, k1, k2, m_r, _, _ = G.pack([real])
    m_d = G.pack([decoy])[5]
    exp, dexp = G.reference("min_tri_below_accepted"), MC.run_reference(decoy)
    assert exp["status"] == R.OK_F and not np.array_equal(exp["inliers_f"], dexp["inliers_f"])
    n1 = len(k1)
    nwork = ex._lib.hs_monoinit_work_bytes(1, n1, G.bound([real]))

    def scene():
        def call(ptr, stream):
            N.check(ex._h, ex._lib.hs_monoinit_estimate_device(ex._h, 1, G.p(par), G.p(off1), ptr["kps1"], G.p(off2), ptr["kps2"], ptr["matches"], None, 0, ptr["results"],
                                                               ptr["inl_h"], ptr["inl_f"], ptr["p3d"], ptr["tri"], ptr["work"], stream))
        return [SO.Step("monoinit_estimate", dict(kps1=(k1, k1.copy()), kps2=(k2, k2.copy()), matches=(m_r, m_d)),
                        dict(results=N.MONOINIT_RESULT_DTYPE.itemsize, inl_h=n1, inl_f=n1, p3d=12 * n1, tri=n1), call,
                        dict(inl_f=[(0, exp["inliers_f"], dexp["inliers_f"])]), work=dict(work=nwork))]

    for steps, got, after in SO.run(ex, scene, tag="hs_monoinit_estimate_device"):
        SO.check(steps, got, after, "hs_monoinit_estimate_device")
        res = got[0]["results"].view(N.MONOINIT_RESULT_DTYPE)[0]
        assert int(res["status"]) == R.OK_F and G.MH.same(res["R21"], exp["R21"]) and int(res["n_triangulated"]) == exp["n_triangulated"]


def test_refused_calls_leave_the_outputs_alone(ex):
    """with a real handle: every refusal is HS_ERR_INVALID before anything is enqueued, and no output byte changes, in both forms; the device form
    also refuses a missing or misaligned work area and misaligned key points"""
    from hyslam_amd import _native as N
    c = MC.cases()["n64"]
    par, off1, off2, k1, k2, m, _, _ = G.pack([c])
    n1 = len(k1)
    res = np.full(N.MONOINIT_RESULT_DTYPE.itemsize, G.FILL, np.uint8)
    ih, jf, tri, p3d = np.full(n1, G.FILL, np.uint8), np.full(n1, G.FILL, np.uint8), np.full(n1, G.FILL, np.uint8), np.full(12 * n1, G.FILL, np.uint8)
    p = G.p

    def variants():
        for field, value in (("max_iterations", 0), ("max_iterations", N.HS_MONOINIT_MAX_ITERATIONS + 1), ("sigma", 0.0), ("fx", -1.0), ("min_parallax_deg", 0.0),
                             ("min_parallax_deg", 180.0), ("min_frac_triangulated", np.nan), ("min_triangulated", -1)):
            bad = par.copy()
            bad[field] = value
            yield 1, bad, off1, off2, 0
        yield 0, par, off1, off2, 0
        yield 1, par, off1[::-1].copy(), off2, 0
        yield 1, par, off1, np.array([-1, len(k2)], np.int64), 0
        yield 1, par, np.array([0, 1 << 31], np.int64), off2, 0    # a frame of 2^31 key points: refused before anything is read
        yield 1, par, off1, off2, 1                                # draw_cap without a table
        yield 1, par, off1, off2, -1

    for Q, pp, o1, o2, cap in variants():
        st = ex._lib.hs_monoinit_estimate(ex._h, Q, p(pp), p(o1), p(k1), p(o2), p(k2), p(m), None, cap, p(res), p(ih), p(jf), p(p3d), p(tri))
        assert st == N.HS_ERR_INVALID, (Q, cap)
    for knock in range(5):
        outs = [p(res), p(ih), p(jf), p(p3d), p(tri)]
        outs[knock] = None
        assert ex._lib.hs_monoinit_estimate(ex._h, 1, p(par), p(off1), p(k1), p(off2), p(k2), p(m), None, 0, *outs) == N.HS_ERR_INVALID
    assert ex._lib.hs_monoinit_estimate(ex._h, 1, p(par), p(off1), None, p(off2), p(k2), p(m), None, 0, p(res), p(ih), p(jf), p(p3d), p(tri)) == N.HS_ERR_INVALID
    assert ex._lib.hs_monoinit_estimate(ex._h, 1, p(par), p(off1), p(k1), p(off2), p(k2), None, None, 0, p(res), p(ih), p(jf), p(p3d), p(tri)) == N.HS_ERR_INVALID
    assert all((a == G.FILL).all() for a in (res, ih, jf, p3d, tri))
    # the device form
    d_k1, d_k2, d_m = hipmem.DevBuf.from_numpy(k1), hipmem.DevBuf.from_numpy(k2), hipmem.DevBuf.from_numpy(m)
    d_res, d_ih, d_if, d_p3d, d_tri = G.out_buf(res.nbytes), G.out_buf(n1), G.out_buf(n1), G.out_buf(12 * n1), G.out_buf(n1)
    nwork = ex._lib.hs_monoinit_work_bytes(1, n1, G.bound([c]))
    d_work = G.out_buf(nwork)
    dev = lambda Q, pp, o1, o2, cap, pk1, pk2, work: ex._lib.hs_monoinit_estimate_device(ex._h, Q, p(pp), p(o1), pk1, p(o2), pk2, d_m.ptr, None, cap, d_res.ptr, d_ih.ptr,
                                                                                         d_if.ptr, d_p3d.ptr, d_tri.ptr, work, None)
    for Q, pp, o1, o2, cap in variants():
        assert dev(Q, pp, o1, o2, cap, d_k1.ptr, d_k2.ptr, d_work.ptr) == N.HS_ERR_INVALID, (Q, cap)
    for pk1, pk2, work in ((d_k1.ptr + 8, d_k2.ptr, d_work.ptr), (d_k1.ptr, d_k2.ptr + 8, d_work.ptr), (d_k1.ptr, d_k2.ptr, None), (d_k1.ptr, d_k2.ptr, d_work.ptr + 8)):
        assert dev(1, par, off1, off2, 0, pk1, pk2, work) == N.HS_ERR_INVALID, "alignment"
    hipmem.sync()
    assert all((G.read(b, np.uint8, n) == G.FILL).all() for b, n in ((d_res, res.nbytes), (d_ih, n1), (d_if, n1), (d_p3d, 12 * n1), (d_tri, n1), (d_work, nwork)))
    assert dev(1, par, off1, off2, 0, d_k1.ptr, d_k2.ptr, d_work.ptr) == N.HS_OK                     # and the call they refused is a valid one
    hipmem.sync()
    assert G.read(d_res, N.MONOINIT_RESULT_DTYPE, 1)["status"][0] == G.reference("n64")["status"]
