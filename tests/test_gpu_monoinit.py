"""GPU: the monocular initialisation — hs_monoinit_estimate(_device) and hyslam_amd.MonoEstimator — against the LITERAL reference of
tests/ref_monoinit.py (pinned by tests/test_monoinit_ref.py) on the cases of tests/monoinit_cases.py.

The host, the device and the Python form must EQUAL the reference: status, scores, iterations, H21 / F21, both masks, n_good, cos_parallax, R21, t21,
p3d and triangulated, float for float (tests/monoinit_host.py).  Outputs start from a 0x55 fill with guard bytes behind them."""
import numpy as np
import pytest

import hipmem
import monoinit_cases as MC
import monoinit_gpu as G
import monoinit_host as MH
import ref_monoinit as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex(gpu):
    import hyslam_amd as HS
    return HS.ORBExtractor(device=0)


@pytest.fixture(scope="module")
def stream(gpu):
    return hipmem.Stream(non_blocking=True)


def run(form, ex, cases, stream):
    return G.run_host(ex, cases) if form == "host" else G.run_device(ex, cases, stream)


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", sorted(MC.cases()))
def test_case_equals_the_reference(ex, stream, name, form):
    c = MC.cases()[name]
    ref = G.reference(name)
    if c["expect"] is not None:
        assert ref["status"] == c["expect"], (name, "the scene does not do what it was built for", ref["status"])
    G.compare_call(name, [c], [ref], run(form, ex, [c], stream))


@pytest.mark.parametrize("form", ["host", "device"])
def test_three_problems_one_of_them_too_few(ex, stream, form):
    cases = MC.batch_q3()
    refs = [G.reference(n) for n in ("outliers_30", "n7_too_few", "plane_h")]
    assert [r["status"] for r in refs] == [R.OK_F, R.TOO_FEW, R.OK_H] and len({r["n_matches"] for r in refs}) == 3
    G.compare_call("Q=3", cases, refs, run(form, ex, cases, stream))


@pytest.mark.parametrize("form", ["host", "device"])
def test_seeded_sweep_in_one_call_of_two_launch_groups(ex, stream, form):
    names = sorted(MC.sweep())
    cases, refs = [MC.sweep()[n] for n in names], [G.reference(n) for n in names]
    assert len(cases) == 32 and {R.FAILED, R.OK_H, R.OK_F} <= {r["status"] for r in refs}
    G.compare_call("sweep", cases, refs, run(form, ex, cases, stream))


def test_second_call_on_the_same_handle_gives_the_same_bytes(ex, stream):
    cases = [MC.cases()[n] for n in ("plane_h", "directed_draws", "outliers_30")]
    first = [a.tobytes() for a in G.run_host(ex, cases)]
    G.run_host(ex, [MC.cases()["general_f"]])                     # another call in between: the scratch holds its leftovers
    assert [a.tobytes() for a in G.run_host(ex, cases)] == first
    assert [a.tobytes() for a in G.run_device(ex, cases, stream)] == first


@pytest.mark.parametrize("form", ["host", "device"])
def test_the_other_layout_of_stage_two_gives_the_same_bytes(ex, stream, form):
    """hs_debug_monoinit_layout(1): one lane per hypothesis instead of one wave.  Cases around its 64-hypothesis workgroups and its LDS chunk of
    matches, a NaN scene, a TOO_FEW problem and directed draws in one batch: EQUAL to LITERAL like the default layout"""
    names = ["its1", "its63", "its64", "its65", "its200", "chi_chunk-1", "chi_chunk+0", "chi_chunk+1", "plane_h", "identical_points", "n7_too_few", "directed_draws", "n8"]
    cases, refs = [MC.cases()[n] for n in names], [G.reference(n) for n in names]
    assert ex._lib.hs_debug_monoinit_layout(1) == 0
    try:
        out = run(form, ex, cases, stream)
    finally:
        assert ex._lib.hs_debug_monoinit_layout(0) == 1
    G.compare_call("lane per hypothesis", cases, refs, out)
    assert ex._lib.hs_debug_monoinit_layout(7) == 0                # anything else changes nothing


def test_python_mirror(ex, stream):
    """hyslam_amd.MonoEstimator: Initialize, initialize_batch and the enqueue-only device form against the reference"""
    import hyslam_amd as HS
    from hyslam_amd import _native as N
    names = ["general_f", "plane_h", "n7_too_few", "directed_draws", "pure_rotation"]

    def make(n):
        c = MC.cases()[n]
        pp = c["params"]
        return HS.MonoEstimator(c["kps1"], (pp["fx"], pp["fy"], pp["cx"], pp["cy"]), sigma=pp["sigma"], MaxIterations=pp["max_iterations"],
                                minTriangulated=pp["min_triangulated"], minFracTriangulated=pp["min_frac_triangulated"], minParallax=pp["min_parallax_deg"], seed=pp["seed"],
                                draws=c["draws"], extractor=ex)

    alone = [make(n).Initialize(MC.cases()[n]["kps2"], MC.cases()[n]["matches12"]) for n in names]
    ests = [make(n) for n in names]
    together = HS.MonoEstimator.initialize_batch(ests, [MC.cases()[n]["kps2"] for n in names], [MC.cases()[n]["matches12"] for n in names])
    for n, a, b, e in zip(names, alone, together, ests):
        ref = G.reference(n)
        ok = ref["status"] in (R.OK_H, R.OK_F)
        for got in (a, b):
            assert got[0] == ok and (got[1] is not None) == ok, n
            MH.compare(n, got[5], e.inliers_h, e.inliers_f, got[3], got[4].astype(np.uint8), ref)
            if ok:
                assert MH.same(got[1], ref["R21"]) and MH.same(got[2], ref["t21"]), n
        if ok:
            assert abs(HS.MonoEstimator.parallax_deg(a[5]) - np.degrees(np.arccos(np.float64(ref["cos_parallax"])))) < 1e-9
    # the enqueue-only form on caller-owned device memory, on a caller's stream
    cases = [MC.cases()[n] for n in names]
    par, off1, off2, kps1, kps2, matches, _, _ = G.pack(cases)
    draws, cap = HS.MonoEstimator.draws_table(ests)
    assert cap == len(MC.cases()["directed_draws"]["draws"]) and draws.shape == (len(names), cap, N.HS_MONOINIT_DRAW_STRIDE)
    Q, n1 = len(names), len(kps1)
    nwork = HS.MonoEstimator.work_bytes(ests, n1)
    assert nwork == ex._lib.hs_monoinit_work_bytes(Q, n1, G.bound(cases))
    d_k1, d_k2, d_m, d_draws = (hipmem.DevBuf.from_numpy(a) for a in (kps1, kps2, matches, draws))
    d_res, d_ih, d_if = G.out_buf(Q * N.MONOINIT_RESULT_DTYPE.itemsize), G.out_buf(n1), G.out_buf(n1)
    d_p3d, d_tri, d_work = G.out_buf(12 * n1), G.out_buf(n1), G.out_buf(nwork)
    HS.MonoEstimator.initialize_batch_device(ests, d_k1, off1, d_k2, off2, d_m, d_res, d_ih, d_if, d_p3d, d_tri, d_work, d_draws=d_draws, draw_cap=cap, stream=stream)
    stream.synchronize()
    G.compare_call("device form of the Python class", cases, [G.reference(n) for n in names],
                   (G.read(d_res, N.MONOINIT_RESULT_DTYPE, Q), G.read(d_ih, np.uint8, n1), G.read(d_if, np.uint8, n1), G.read(d_p3d, np.float32, 3 * n1).reshape(n1, 3),
                    G.read(d_tri, np.uint8, n1)))


def test_end_to_end_from_search_for_initialization(ex):
    """matches12 as hs_search_for_initialization leaves it, handed to MonoEstimator unchanged: equal to the reference on the same arrays"""
    import hyslam_amd as HS
    import oracle
    from hyslam_amd import _native as N
    from test_oracle_matchers import mono_init_scene
    k1, d1, fa, prev = mono_init_scene(51, 1000)
    Fg, keep = oracle.make_frame_view(N.FrameView, **fa)
    matcher = HS.FeatureMatcher(HS.FeatureMatcherSettings(nnratio=0.8, TH_LOW=50.0), extractor=ex)
    m12, _, n = matcher.SearchForInitialization(k1, d1, Fg, prev, 100)
    assert n > 100 and len(m12) == len(k1)
    est = HS.MonoEstimator(k1, (500.0, 500.0, 320.0, 240.0), MaxIterations=20, seed=5, extractor=ex)
    got = est.Initialize(fa["kps"], m12)
    xy = lambda k: np.stack([k["x"], k["y"]], 1)
    ref = R.estimate(xy(k1), xy(fa["kps"]), m12, dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0, max_iterations=20, seed=5))
    assert ref["n_matches"] == n
    MH.compare("end to end", got[5], est.inliers_h, est.inliers_f, got[3], got[4].astype(np.uint8), ref)
