"""GPU: the batched EPnP RANSAC — hs_pnp_iterate(_device) and hyslam_amd.PnPsolver — against LITERAL of tests/ref_pnp.py in point order (pinned by
tests/test_pnp_ref.py) on the cases of tests/pnp_cases.py.

Exact: status, n_inliers, the masks, at_iteration, iterations, hypotheses_run, refines_run and the state (iterations, best_inliers, best_Tcw, the best
mask).  Tcw_d: the device sums in LITERAL's order and every operation on both sides is a correctly rounded IEEE double operation, so it is tested for
EQUALITY; Tcw is float32(Tcw_d) bit for bit.  Outputs start from a 0x55 fill with guard bytes behind them: a mask that is "not touched" still
holds it."""
import ctypes as C

import numpy as np
import pytest

import hipmem
import pnp_cases as PC
import ref_pnp as R

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0x55


@pytest.fixture(scope="module")
def ex(gpu):
    import hyslam_amd as HS
    return HS.ORBExtractor(device=0)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def pack(cases):
    """the arrays of one call over `cases`: params [Q], offsets [Q + 1], corrs, draws [Q, cap, MAX_SET] or None, cap.  A table shorter than the call's
    cap is continued with the generator's own words, which is what draw_cap < it means for that problem."""
    from hyslam_amd import _native as N
    Q = len(cases)
    par = np.zeros(Q, N.PNP_PARAMS_DTYPE)
    for q, c in enumerate(cases):
        for k in ("probability", "min_inliers", "max_iterations", "min_set", "epsilon", "th2", "seed"):
            par[k][q] = c["params"][k]
        par["fx"][q], par["fy"][q], par["cx"][q], par["cy"][q] = c["cam"]
    off = np.zeros(Q + 1, np.int64)
    off[1:] = np.cumsum([len(c["corrs"]) for c in cases])
    corrs = np.concatenate([np.ascontiguousarray(c["corrs"]).view(N.PNP_CORR_DTYPE) for c in cases])
    cap = max([0] + [len(c["draws"]) for c in cases if c["draws"] is not None])
    draws = None
    if cap:
        draws = np.zeros((Q, cap, R.MAX_SET), np.uint32)
        for q, c in enumerate(cases):
            ms = c["params"]["min_set"]
            for it in range(cap):
                draws[q, it, :ms] = [R.draw32(c["params"]["seed"], it, k, ms, c["draws"]) for k in range(ms)]
    return par, off, corrs, draws, cap


def fresh(cases):
    from hyslam_amd import _native as N
    n = sum(len(c["corrs"]) for c in cases)
    return np.zeros(len(cases), N.PNP_STATE_DTYPE), np.full(n, FILL, np.uint8)


def run_host(ex, cases, n_iterations, states, best):
    """the C ABI host form on sentinel-filled outputs with guards -> (results, inlier masks); states and best are updated in place"""
    from hyslam_amd import _native as N
    par, off, corrs, draws, cap = pack(cases)
    Q, n = len(cases), len(corrs)
    inl = np.full(n + GUARD, FILL, np.uint8)
    res = np.full(Q * N.PNP_RESULT_DTYPE.itemsize + GUARD, FILL, np.uint8)
    N.check(ex._h, ex._lib.hs_pnp_iterate(ex._h, Q, p(par), p(off), p(corrs), n_iterations, p(draws) if cap else None, cap, p(states), p(best), p(res), p(inl)))
    assert (inl[n:] == FILL).all() and (res[Q * N.PNP_RESULT_DTYPE.itemsize:] == FILL).all(), "bytes written behind the output"
    return res[:Q * N.PNP_RESULT_DTYPE.itemsize].view(N.PNP_RESULT_DTYPE).copy(), inl[:n].copy()


def out_buf(nbytes):
    b = hipmem.DevBuf(nbytes + GUARD)
    b.fill(FILL)
    return b


def guarded(a):
    a = np.ascontiguousarray(a)
    b = out_buf(a.nbytes)
    if a.nbytes:
        hipmem._ok(hipmem.hip().hipMemcpy(b.ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")
    return b


def read(buf, dtype, count):
    nbytes = np.dtype(dtype).itemsize * count
    raw = buf.to_numpy(np.uint8, nbytes + GUARD)
    assert (raw[nbytes:] == FILL).all(), "bytes written behind the output"
    return raw[:nbytes].view(dtype).copy()


def run_device(ex, cases, n_iterations, states, best, stream):
    """the device form on a caller's stream; the work area is the size hs_pnp_work_bytes gives and guarded too"""
    from hyslam_amd import _native as N
    par, off, corrs, draws, cap = pack(cases)
    Q, n = len(cases), len(corrs)
    H = max([n_iterations] + [int(c["params"]["max_iterations"]) for c in cases])
    nwork = ex._lib.hs_pnp_work_bytes(Q, n, H)
    d_corrs, d_draws = hipmem.DevBuf.from_numpy(corrs), (hipmem.DevBuf.from_numpy(draws) if cap else None)
    d_states, d_best = guarded(states), guarded(best)
    d_res, d_inl, d_work = out_buf(Q * N.PNP_RESULT_DTYPE.itemsize), out_buf(n), out_buf(nwork)
    N.check(ex._h, ex._lib.hs_pnp_iterate_device(ex._h, Q, p(par), p(off), d_corrs.ptr, n_iterations, d_draws.ptr if cap else None, cap, d_states.ptr, d_best.ptr,
                                                 d_res.ptr, d_inl.ptr, d_work.ptr, stream.ptr))
    stream.synchronize()
    read(d_work, np.uint8, nwork)
    states[:] = read(d_states, N.PNP_STATE_DTYPE, Q)
    best[:] = read(d_best, np.uint8, n)
    return read(d_res, N.PNP_RESULT_DTYPE, Q), read(d_inl, np.uint8, n)


def compare(tag, res, state, best, inl, exp, state_before):
    """one problem of one call against LITERAL's (result, state after)"""
    r, st = exp
    got = (int(res["status"]), int(res["n_inliers"]), int(res["at_iteration"]), int(res["iterations"]), int(res["hypotheses_run"]), int(res["refines_run"]))
    want = (r["status"], r["n_inliers"], r["at_iteration"], r["iterations"], r["hypotheses_run"], r["refines_run"])
    assert got == want, (tag, "status, n_inliers, at_iteration, iterations, hypotheses_run, refines_run", got, want)
    if r["status"] == R.TOO_FEW:
        assert state.tobytes() == state_before.tobytes() and (best == FILL).all(), (tag, "TOO_FEW touched the state")
    else:
        assert (int(state["iterations"]), int(state["best_inliers"])) == (st["iterations"], st["best_inliers"]), (tag, "state")
        if st["best_inliers"] > 0:
            assert np.array_equal(best, st["best_mask"]), (tag, "best mask")
            assert np.array_equal(state["best_Tcw"].reshape(4, 4), st["best_Tcw"]), (tag, "best_Tcw")
    if r["mask"] is None:
        assert (inl == FILL).all(), (tag, "the inlier mask of a call without a pose was touched")
    else:
        assert np.array_equal(inl, r["mask"]), (tag, "inlier mask", int((inl != r["mask"]).sum()))
        d = np.abs(res["Tcw_d"].reshape(4, 4) - r["Tcw_d"])
        print("%s: largest |Tcw_d - LITERAL| = %.3g" % (tag, float(d.max())))
        assert np.array_equal(res["Tcw_d"].reshape(4, 4), r["Tcw_d"]), (tag, "Tcw_d differs from LITERAL", float(d.max()))
    assert np.array_equal(res["Tcw"], res["Tcw_d"].astype(np.float32)), (tag, "Tcw is not float32(Tcw_d)")
    assert np.array_equal(res["Tcw"].reshape(4, 4), r["Tcw"]), (tag, "Tcw")


def run_case(ex, names, runner, calls=None):
    """every call of the named cases (all of one length) in one batch -> the per-call (results, inlier, states, best) for further checks"""
    cases = [PC.cases()[n] for n in names]
    off = np.concatenate([[0], np.cumsum([len(c["corrs"]) for c in cases])])
    states, best = fresh(cases)
    out = []
    for k, n_it in enumerate(calls or cases[0]["calls"]):
        before = states.copy()
        res, inl = runner(ex, cases, n_it, states, best)
        for q, name in enumerate(names):
            compare("%s call %d" % (name, k), res[q], states[q], best[off[q]:off[q + 1]], inl[off[q]:off[q + 1]], PC.expected(name)[k], before[q])
        out.append((res.copy(), inl.copy(), states.copy(), best.copy()))
    return out


SINGLE = sorted(PC.cases())


@pytest.mark.parametrize("name", SINGLE)
def test_case_against_literal_host_form(ex, name):
    run_case(ex, [name], run_host)


def test_three_problems_of_different_size_in_one_call(ex):
    assert len({len(PC.cases()[n]["corrs"]) for n in PC.BATCH}) == 3 and PC.expected("n9_too_few")[0][0]["status"] == R.TOO_FEW
    run_case(ex, list(PC.BATCH), run_host)


def test_seventeen_problems_take_two_launch_pairs(ex):
    assert len(PC.BATCH17) == 17 and all(PC.cases()[n]["calls"][0] == 12 or n == "n9_too_few" for n in PC.BATCH17)
    run_case(ex, list(PC.BATCH17), run_host)


def test_refine_points_through_the_work_area(ex):
    """N = 1100 > the 1024 correspondences k_pnp_select keeps in LDS: host form and device form (whose work area is guarded and exactly as large as stated)"""
    c = PC.cases()["n1100_work_area"]
    (res, _, _, _), = run_case(ex, ["n1100_work_area"], run_host)
    assert len(c["corrs"]) == 1100 and res["status"][0] == R.REFINED and int(res["n_inliers"][0]) > 700 and int(res["at_iteration"][0]) == 2
    stream = hipmem.Stream(non_blocking=True)
    # behind another problem, so that its points start at 5 * off of the area; n = 4 leaves n65 its planned 12 iterations and its expected result
    run_case(ex, ["n65", "n1100_work_area"], lambda *a: run_device(*a, stream), calls=[4])


def test_the_loop_condition_is_an_or(ex):
    (a, _, _, _), = run_case(ex, ["or_max3_n5"], run_host)
    (b, _, _, _), = run_case(ex, ["or_max12_n5"], run_host)
    assert (int(a["iterations"][0]), int(a["hypotheses_run"][0])) == (5, 5) and (int(b["iterations"][0]), int(b["hypotheses_run"][0])) == (12, 12)


def test_second_calls(ex):
    first, second = run_case(ex, ["again_after_refined"], run_host)
    assert first[0]["status"][0] == second[0]["status"][0] == R.REFINED
    assert first[0]["Tcw_d"][0].tobytes() == second[0]["Tcw_d"][0].tobytes() and np.array_equal(first[1], second[1]), "the same refined pose again"
    assert int(second[0]["at_iteration"][0]) > int(first[0]["at_iteration"][0]) and int(second[0]["refines_run"][0]) == 1
    first, second = run_case(ex, ["again_after_failed_refine"], run_host)
    assert first[0]["status"][0] == second[0]["status"][0] == R.BEST and int(second[0]["refines_run"][0]) == 1, "the failed refine is evaluated again, and fails again"
    first, second = run_case(ex, ["again_exhausted"], run_host)
    assert (int(first[0]["iterations"][0]), int(second[0]["iterations"][0]), int(second[0]["hypotheses_run"][0])) == (4, 7, 3)


def test_outcomes(ex):
    (none, inl, _, _), = run_case(ex, ["or_max12_n5"], run_host)
    assert none["status"][0] == R.NONE and (inl == FILL).all()
    (best, _, st, _), _ = run_case(ex, ["best_refine_lands_on_min"], run_host)
    c = PC.cases()["best_refine_lands_on_min"]
    min_inl = R.plan(len(c["corrs"]), **c["params"])[0]
    assert best["status"][0] == R.BEST and int(best["n_inliers"][0]) == min_inl and int(best["refines_run"][0]) >= 1
    (nf, _, _, _), = run_case(ex, ["nonfinite_corr"], run_host)
    assert int(nf["status"][0]) in (R.TOO_FEW, R.REFINED, R.BEST, R.NONE, R.NONFINITE)


def test_directed_draws_then_the_generator(ex):
    c = PC.cases()["directed_draws"]
    assert len(c["draws"]) == 4 < c["calls"][0]
    s = PC.solver(c)
    assert s.hypothesis(0)[1][4][0] == len(c["corrs"]) - 1, "the first draw of the table takes the last index"
    assert len(set(s.hypothesis(2)[1][4])) == len(set(s.hypothesis(3)[1][4])) == 4, "repeated words take different correspondences"
    run_case(ex, ["directed_draws"], run_host)
    # without the table the generator alone decides, and the counts of the first iterations differ
    plain = dict(c, draws=None)
    states, best = fresh([plain])
    res, _ = run_host(ex, [plain], 12, states, best)
    r = R.Solver(plain["corrs"], plain["cam"], plain["params"], None).iterate(12)
    assert (int(res["status"][0]), int(res["n_inliers"][0]), int(res["at_iteration"][0])) == (r["status"], r["n_inliers"], r["at_iteration"])


def test_host_and_device_forms_twice_under_poison_give_the_same_bytes(ex):
    """host form == device form == the same call again == the call behind hs_debug_poison, byte for byte, over a batch with a second call"""
    from hyslam_amd import _native as N
    names = ["n65", "again_after_refined", "n9_too_few", "best_refine_lands_on_min"]
    cases = [PC.cases()[n] for n in names]

    def both_calls(runner):
        states, best = fresh(cases)
        out = []
        for n_it in (12, 3):
            res, inl = runner(ex, cases, n_it, states, best)
            out.append((res.tobytes(), inl.tobytes(), states.tobytes(), best.tobytes()))
        return out

    host = both_calls(run_host)
    stream = hipmem.Stream(non_blocking=True)
    assert both_calls(lambda *a: run_device(*a, stream)) == host, "device form differs from host form"
    assert both_calls(run_host) == host, "the same call twice differs"
    try:
        assert ex._lib.hs_debug_poison(0xA7) == N.HS_OK
        assert both_calls(run_host) == host, "the result depends on what the scratch held"
    finally:
        ex._lib.hs_debug_poison(-1)


def test_device_form_behind_a_pending_write_of_its_inputs(ex):
    """the device form on a caller's stream: the real inputs arrive behind a delay on that stream, the outputs are snapshotted right behind the call"""
    import stream_order as SO
    from hyslam_amd import _native as N
    real, decoy = PC.cases()["n65"], PC.cases()["n64"]
    decoy = dict(decoy, corrs=np.concatenate([decoy["corrs"], decoy["corrs"][:1]]))          # the decoy at the real case's size: valid, and another answer
    n, H = 65, 12
    par, off, corrs_r, _, _ = pack([real])
    _, _, corrs_d, _, _ = pack([decoy])
    exp = R.Solver(real["corrs"], real["cam"], real["params"], None).iterate(12)
    dexp = R.Solver(decoy["corrs"], real["cam"], real["params"], None).iterate(12)              # the decoy's correspondences under the call's parameters
    assert exp["status"] == R.REFINED and not np.array_equal(exp["mask"], dexp["mask"] if dexp["mask"] is not None else np.zeros(n, np.uint8))
    st0, _ = fresh([real])
    nwork = ex._lib.hs_pnp_work_bytes(1, n, H)

    def scene():
        def call(ptr, stream):
            N.check(ex._h, ex._lib.hs_pnp_iterate_device(ex._h, 1, p(par), p(off), ptr["corrs"], 12, None, 0, ptr["states"], ptr["best"], ptr["results"], ptr["inl"],
                                                         ptr["work"], stream))
        want = lambda e: e["mask"] if e["mask"] is not None else np.full(n, SO.FILL_OUT, np.uint8)
        return [SO.Step("pnp_iterate", dict(corrs=(corrs_r, corrs_d), states=(st0, st0.copy())), dict(results=N.PNP_RESULT_DTYPE.itemsize, inl=n, best=n), call,
                        dict(inl=[(0, want(exp), want(dexp))]), work=dict(work=nwork))]

    for steps, got, after in SO.run(ex, scene, tag="hs_pnp_iterate_device"):
        SO.check(steps, got, after, "hs_pnp_iterate_device")
        res = got[0]["results"].view(N.PNP_RESULT_DTYPE)[0]
        assert int(res["status"]) == R.REFINED and np.array_equal(res["Tcw_d"].reshape(4, 4), exp["Tcw_d"])


def test_iterate_batch_equals_iterate_alone(ex):
    import hyslam_amd as HS
    names = ["n64", "n12", "n9_too_few", "directed_draws"]

    def make():
        out = []
        for n in names:
            c = PC.cases()[n]
            s = HS.PnPsolver(c["cam"], corrs=c["corrs"], seed=c["params"]["seed"], draws=c["draws"], extractor=ex)
            pp = c["params"]
            s.SetRansacParameters(pp["probability"], pp["min_inliers"], pp["max_iterations"], pp["min_set"], pp["epsilon"], pp["th2"])
            out.append(s)
        return out

    alone = [s.iterate(12) for s in make()]
    together = HS.PnPsolver.iterate_batch(make(), 12)
    for n, a, b in zip(names, alone, together):
        r = PC.expected(n)[0][0]
        assert (a[0] is None) == (b[0] is None) == (r["mask"] is None) and a[1] == b[1] == (r["status"] != R.REFINED) and a[3] == b[3] == r["n_inliers"], n
        if a[0] is not None:
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], r["Tcw"]) and np.array_equal(a[2], b[2]), n
            flags = np.zeros(len(a[2]), bool)
            flags[PC.cases()[n]["corrs"]["kp"][r["mask"] != 0]] = True
            assert np.array_equal(a[2], flags), (n, "vbInliers is indexed by keypoint")


def test_refused_calls_leave_the_outputs_alone(ex):
    """with a real handle: every refusal is HS_ERR_INVALID before anything is enqueued, and no output byte changes"""
    from hyslam_amd import _native as N
    c = PC.cases()["n12"]
    par, off, corrs, _, _ = pack([c])
    states, best = fresh([c])
    inl, res = np.full(len(corrs), FILL, np.uint8), np.full(N.PNP_RESULT_DTYPE.itemsize, FILL, np.uint8)
    small = par.copy(); small["min_set"] = 3
    for args in ((0, par, off, corrs, 5), (1, par, off, corrs, 0), (1, par, off, corrs, -1), (1, small, off, corrs, 5), (1, par, off[::-1].copy(), corrs, 5),
                 (1, None, off, corrs, 5), (1, par, None, corrs, 5), (1, par, off, None, 5)):
        Q, pp, po, pc, n = args
        st = ex._lib.hs_pnp_iterate(ex._h, Q, p(pp) if pp is not None else None, p(po) if po is not None else None, p(pc) if pc is not None else None, n, None, 0,
                                    p(states), p(best), p(res), p(inl))
        assert st == N.HS_ERR_INVALID, args[0:1] + args[4:]
    assert ex._lib.hs_pnp_iterate(ex._h, 1, p(par), p(off), p(corrs), 5, None, 1, p(states), p(best), p(res), p(inl)) == N.HS_ERR_INVALID, "draw_cap without a table"
    neg = states.copy()
    neg["iterations"] = -1
    assert ex._lib.hs_pnp_iterate(ex._h, 1, p(par), p(off), p(corrs), 5, None, 0, p(neg), p(best), p(res), p(inl)) == N.HS_ERR_INVALID, "a state with a negative count"
    assert (inl == FILL).all() and (res == FILL).all() and (best == FILL).all() and not states.view(np.uint8).any()


def test_relocalisation_end_to_end_on_synth(ex):
    """landmarks seen from a known pose (hyslam_amd.synth.synth_local_map), 40 % of the matches pointed at another landmark: PnPsolver finds the pose and the
    inliers, Optimizer.PoseOptimization refines it on those; the result is the pose the numpy references of both stages give"""
    import hyslam_amd as HS
    import poseopt_cases as PP
    import ref_poseopt as RP
    from hyslam_amd import _native as N, synth
    n, seed = 200, 32
    U = lambda s: PC.uniform(seed, n, s)
    kps = np.zeros(n, N.KP_DTYPE)
    kps["x"], kps["y"], kps["size"] = 20 + 600 * U(1), 20 + 440 * U(2), 31.0
    Rcw, tcw = PC.rotation(seed).astype(np.float32), (PC.uniform(seed, 3, 91) - 0.5).astype(np.float32)
    cam = [float(c) for c in PC.CAM]
    lms = synth.synth_local_map(kps, np.zeros((n, 32), np.uint8), np.full(n, -1.0), n, seed, *cam, Rcw, tcw)
    matches, wrong = np.arange(n), U(3) < 0.4
    matches[wrong] = (matches[wrong] + 17) % n
    assert 0.3 * n < wrong.sum() < 0.5 * n
    solver = HS.PnPsolver(cam, kps=kps, landmarks=lms, matches=matches, seed=5, extractor=ex)
    solver.SetRansacParameters(0.99, 10, 12, 4, 0.4, 5.991)
    Tcw, no_more, flags, n_inl = solver.iterate(12)
    ref = R.Solver(HS.PnPsolver.correspondences(kps, lms, matches), PC.CAM, dict(R.DEFAULT, max_iterations=12, seed=5, epsilon=0.4)).iterate(12)
    assert ref["status"] == R.REFINED and Tcw is not None and not no_more and n_inl == ref["n_inliers"] > 0.55 * n
    assert np.array_equal(Tcw, ref["Tcw"]) and np.array_equal(np.nonzero(flags)[0], np.nonzero(ref["mask"])[0]) and not (flags & wrong).any()
    assert np.abs(Tcw[:3, :3] - Rcw).max() < 5e-3 and np.abs(Tcw[:3, 3] - tcw).max() < 5e-2, "EPnP over the inliers is near the known pose"
    kp_lm = np.where(flags, matches, -1).astype(np.int32)
    cam5, uR = cam + [0.0], np.full(n, -1.0, np.float32)
    pose, outlier, n_good = HS.Optimizer(extractor=ex).PoseOptimization(Tcw, cam5, kps=kps, uR=uR, kp_lm=kp_lm, landmarks=lms)
    edges, _ = RP.gather_edges(kps, uR, kp_lm, lms["pos"])
    want = RP.pose_optimization_fast(ref["Tcw"], cam5, edges)
    tau = float(PP.load_golden()["tau"])
    assert n_good == want["n_good"] and np.array_equal(outlier[edges["kp"]], want["outlier"])
    assert np.abs(pose.astype(np.float64) - want["Tcw_d"]).max() <= tau + 2.0 ** -23 * max(1.0, np.abs(want["Tcw_d"]).max()), "within tau and the float rounding of Tcw"
    assert np.abs(pose[:3, :3] - Rcw).max() < 5e-3 and np.abs(pose[:3, 3] - tcw).max() < 5e-2
