"""GPU: the batched Horn Sim3 RANSAC — hs_sim3_iterate(_device) and hyslam_amd.Sim3Solver — against the D19 reference of tests/ref_sim3.py (pinned by
tests/test_sim3_ref.py) on the cases of tests/sim3_cases.py.

The host and the device form must EQUAL the reference: status, n_inliers, at_iteration, iterations, hypotheses_run, both masks, and R, t, s and T12 of
the result and of the state, float for float (tests/sim3_gpu.py).  Outputs start from a 0x55 fill with guard bytes behind them."""
import numpy as np
import pytest

import hipmem
import ref_sim3 as R
import sim3_cases as SC
import sim3_gpu as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex(gpu):
    import hyslam_amd as HS
    return HS.ORBExtractor(device=0)


@pytest.fixture(scope="module")
def stream(gpu):
    return hipmem.Stream(non_blocking=True)


def runner(form, stream):
    return G.run_host if form == "host" else (lambda *a: G.run_device(*a, stream))


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", sorted(SC.cases()))
def test_case_equals_the_reference(ex, stream, name, form):
    c = SC.cases()[name]
    G.run_cases(ex, [c], runner(form, stream), c["calls"], tag=name)


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("H", [1, 5, 64, 65, 300])
def test_hypothesis_counts_around_the_wave(ex, stream, H, form):
    """n100_sparse never returns early, so the state's best after the call is the LAST hypothesis that attains the largest count of all H: a lane that
    sampled, solved or counted wrongly anywhere in the range moves it"""
    c = SC.cases()["n100_sparse"]
    (res, _, st, _), = G.run_cases(ex, [c], runner(form, stream), [H], tag="H=%d" % H)
    assert int(res["hypotheses_run"][0]) == H and int(st["iterations"][0]) == H and int(res["status"][0]) == (R.EXHAUSTED if H == 300 else R.CONTINUE)


@pytest.mark.parametrize("form", ["host", "device"])
def test_seventeen_problems_take_two_launch_pairs(ex, stream, form):
    names = sorted(SC.cases())[:17]
    cases = [SC.cases()[n] for n in names]
    assert len(cases) == 17 and len({len(c["corrs"]) for c in cases}) > 5
    G.run_cases(ex, cases, runner(form, stream), [5, 7], tag="Q=17")


def test_one_past_the_staging_chunk(ex, stream):
    c = SC.cases()["n257"]
    assert len(c["corrs"]) == 257
    (res, inl, _, _), = G.run_cases(ex, [c], G.run_host, c["calls"], tag="n257")
    assert int(res["status"][0]) == R.FOUND and inl[256] in (0, 1) and int(inl.sum()) == int(res["n_inliers"][0]) > 150
    # behind another problem, so that its correspondences do not start at the array's first element
    G.run_cases(ex, [SC.cases()["n30_same_camera"], c], runner("device", stream), [7], tag="n30 + n257")


def sweep_cases():
    """about 200 small random problems: N in [0, 40], every parameter seeded"""
    out = []
    for i in range(200):
        u = SC.uniform(1000 + i, 6, 7)
        N = int(u[0] * 41)
        fix = int(u[1] < 0.3)
        mi = int(u[2] * min(N + 2, 14))
        c = SC.case(SC.scene(2000 + i, N, outliers=float(0.1 + 0.6 * u[3]), fix_scale=bool(fix)), dict(seed=int(u[4] * 1e6), fix_scale=fix, min_inliers=mi,
                                                                                                       max_iterations=int(1 + u[5] * 30)),
                    k2=SC.K1 if i % 3 == 0 else SC.K2)
        out.append(c)
    return out


@pytest.mark.parametrize("form", ["host", "device"])
def test_seeded_sweep_of_small_problems(ex, stream, form):
    cases = sweep_cases()
    seen = set()
    for k, n_it in enumerate((3, 7, 12, 20)):
        chunk = cases[50 * k:50 * k + 50]
        for res, _, _, _ in G.run_cases(ex, chunk, runner(form, stream), [n_it, n_it], tag="sweep n=%d" % n_it):
            seen |= set(int(s) for s in res["status"])
    assert {R.TOO_FEW, R.FOUND, R.CONTINUE, R.EXHAUSTED} <= seen, seen


def test_python_mirror(ex):
    """hyslam_amd.Sim3Solver: iterate, iterate_batch, find_batch and the estimates against the reference; vbInliers is mN1 long and scattered through idx1"""
    import hyslam_amd as HS
    names = ["n100", "n100_rounds", "too_few", "n40_fix_scale", "popped_slot"]

    def make():
        out = []
        for n in names:
            c = SC.cases()[n]
            pp = c["params"]
            s = HS.Sim3Solver(c["k1"], c["k2"], c["corrs"], n_matches=2 * len(c["corrs"]) + 3, fix_scale=bool(pp["fix_scale"]), seed=pp["seed"], draws=c["draws"], extractor=ex)
            s.SetRansacParameters(pp["probability"], pp["min_inliers"], pp["max_iterations"])
            out.append(s)
        return out

    alone = [s.iterate(5) for s in make()]
    solvers = make()
    together = HS.Sim3Solver.iterate_batch(solvers, 5)
    for n, a, b, s in zip(names, alone, together, solvers):
        c = SC.cases()[n]
        ref = SC.solver(c)
        r = ref.iterate(5)
        found = r["status"] == R.FOUND
        assert (a[0] is not None) == (b[0] is not None) == found and a[1] == b[1] == (r["status"] in (R.TOO_FEW, R.EXHAUSTED)) and a[3] == b[3] == r["n_inliers"], n
        flags = np.zeros(2 * len(c["corrs"]) + 3, bool)
        flags[c["corrs"]["idx1"][r["mask"] != 0]] = True
        assert len(a[2]) == 2 * len(c["corrs"]) + 3 and np.array_equal(a[2], flags) and np.array_equal(b[2], flags), (n, "vbInliers")
        if found:
            assert np.array_equal(a[0], r["T12"].reshape(4, 4)) and np.array_equal(b[0], a[0]), n
        if ref.best is not None:
            assert G.same(s.GetEstimatedRotation(), ref.best[0]) and G.same(s.GetEstimatedTranslation(), ref.best[1]) and G.same(s.GetEstimatedScale(), ref.best[2]), n
        assert s.max_iterations == ref.max_its
    found = HS.Sim3Solver.find_batch(make())
    for n, f in zip(names, found):
        r = SC.solver(SC.cases()[n]).find()
        assert (f[0] is not None) == (r["status"] == R.FOUND) and f[2] == r["n_inliers"], n
        if f[0] is not None:
            assert np.array_equal(f[0], r["T12"].reshape(4, 4)), n


def test_gathering_as_the_constructor_walks(ex):
    """Sim3Solver.correspondences: ascending i1; a null match, a null own point, a bad point and a negative index on either side are skipped"""
    import hyslam_amd as HS
    from hyslam_amd import _native as N
    L = 8
    pos1 = (SC.uniform(5, 3 * L, 1).reshape(L, 3) * 4 + 1).astype(np.float32)
    pos2 = (SC.uniform(5, 3 * L, 2).reshape(L, 3) * 4 + 1).astype(np.float32)
    kps = np.zeros(10, N.KP_DTYPE)
    kps["size"] = 31.0 * 1.2 ** (np.arange(10) % 4)
    matched12 = np.array([3, -1, 2, 5, 6, 7, 0, 1, 4], np.int64)       # by i1
    points1 = np.array([0, 1, -1, 2, 3, 4, 5, 6, 7], np.int64)
    bad1, bad2 = np.zeros(L, bool), np.zeros(L, bool)
    bad1[2], bad2[6] = True, True                                      # i1 = 3 (own point 2 bad), i1 = 4 (match 6 bad)
    index1, index2 = np.arange(L) % 10, (np.arange(L) + 3) % 10
    index1[4], index2[0] = -1, -1                                      # i1 = 5 (own point 4 not in KF1), i1 = 6 (match 0 not in KF2)
    T1, T2 = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    T1[:3, 3], T2[0, :3] = (0.5, -0.25, 1.0), (0.0, 1.0, 0.0)
    T2[1, :3] = (-1.0, 0.0, 0.0)
    c = HS.Sim3Solver.correspondences(matched12, points1, pos1, pos2, bad1, bad2, index1, index2, kps, kps, T1, T2)
    assert c["idx1"].tolist() == [0, 7, 8]                             # 1: null match, 2: null own point
    assert np.array_equal(c["X1c"], pos1[[0, 6, 7]] + T1[:3, 3]) and np.array_equal(c["X2c"][:, 0], pos2[[3, 1, 4], 1]) and np.array_equal(c["X2c"][:, 1], -pos2[[3, 1, 4], 0])
    lv1, lv2 = index1[[0, 6, 7]] % 4, index2[[3, 1, 4]] % 4
    assert np.allclose(c["sigma2_1"], 1.44 ** lv1, rtol=1e-6) and np.allclose(c["sigma2_2"], 1.44 ** lv2, rtol=1e-6)
