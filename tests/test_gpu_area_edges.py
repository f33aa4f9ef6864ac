"""GPU parity of every grid-area matcher on the edge cases of tests/scenes.py (area_edge_cases, area_size_cases): hs_frame_grid,
hs_search_by_projection_sim3, hs_search_by_sim3, hs_search_by_projection with each preset of the Python mirror (local map, last frame,
keyframe, Fuse) plus its _device and _frame entry points, and hs_search_for_initialization.  Bit-exact against the oracle, and against the
numpy restatement (tests/pyref.py) wherever it runs.  One handle serves every case, so its scratch shrinks and grows between calls."""
import ctypes as C

import numpy as np
import pytest

import hipmem
import oracle
import pyref
import scenes
import hyslam_amd as HS
from hyslam_amd import _native as N

pytestmark = pytest.mark.gpu
f32 = np.float32
PYREF_MAX_N = 2000


@pytest.fixture(scope="module")
def matcher(gpu):
    return HS.FeatureMatcher(HS.FeatureMatcherSettings(nnratio=0.8), HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=500)))


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def presets(m, th):
    """(name, mirror call, oracle hs_proj_params) for each hs_proj_params preset of hyslam_amd.FeatureMatcher"""
    return (
        ("local map", lambda F, l: m.SearchByProjection(F, l, th), oracle.ProjParams(th, m.TH_HIGH, m.mfNNratio, 0.5, 1.5, 1, 1, 0)),
        ("last frame", lambda F, l: m.SearchByProjectionLastFrame(F, l, th), oracle.ProjParams(th, m.TH_HIGH, m.mfNNratio, 0.5, 1.5, 0, 1, 1)),
        ("keyframe", lambda F, l: m.SearchByProjectionKeyFrame(F, l, th, 70), oracle.ProjParams(th, 70.0, 1.0, 0.5, 1.5, 1, 0, 0)),
        ("fuse", lambda F, l: m.Fuse(F, l, th, 5.99),
         oracle.ProjParams(th, m.TH_LOW, 1.0, 0.5, 1.5, use_distance=1, use_stereo=0, check_rotation=0, use_prev_matched=0, use_viewing_angle=1,
                           max_view_angle=1.047, use_reprojection=1, reproj_threshold=5.99, sigma_ref=1.0, first_wins=1)),
    )


def gpu_sim3_projection(m, Fg, case):
    ex = m._ex
    lms = np.ascontiguousarray(case["lms"], N.LM_DTYPE)
    S = np.ascontiguousarray(case["Scw"], f32).reshape(16)
    taken = np.ascontiguousarray(case["kp_matched"], np.uint8).copy()
    midx = np.full(len(lms), -1, np.int32)
    n = C.c_int32()
    N.check(ex._h, ex._lib.hs_search_by_projection_sim3(ex._h, C.byref(Fg), p(S), p(lms), len(lms), int(case["th"]), float(case["th_low"]), p(taken),
                                                        p(midx), C.byref(n)))
    return midx, taken, n.value


def gpu_sim3(m, Fg1, Fg2, s):
    ex = m._ex
    l1, l2 = np.ascontiguousarray(s["lms1"], N.LM_DTYPE), np.ascontiguousarray(s["lms2"], N.LM_DTYPE)
    R, t = np.ascontiguousarray(s["R12"], f32).reshape(9), np.ascontiguousarray(s["t12"], f32).reshape(3)
    out = np.full(Fg1.n, -1, np.int32)
    n = C.c_int32()
    N.check(ex._h, ex._lib.hs_search_by_sim3(ex._h, C.byref(Fg1), p(l1), C.byref(Fg2), p(l2), float(s["s12"]), p(R), p(t), float(s["th"]),
                                             float(s["th_high"]), p(out), C.byref(n)))
    return out, n.value


def gpu_frame_grid(m, Fg):
    ex = m._ex
    got = np.zeros((Fg.n, 2), np.int8)
    N.check(ex._h, ex._lib.hs_frame_grid(ex._h, C.byref(Fg), p(got)))
    return got.astype(np.int64)


def gpu_projection_device(m, fa, lms, pp):
    """hs_search_by_projection_device: every frame array and the landmarks in device memory, on a caller stream"""
    ex = m._ex
    Fg, keep = oracle.make_frame_view(N.FrameView, **fa)
    bufs = [hipmem.DevBuf.from_numpy(np.ascontiguousarray(a)) for a in (fa["kps"], fa["desc"], fa["uR"], fa["kp_lm_obs"], lms)]
    Fg.kps, Fg.desc, Fg.uR, Fg.kp_lm_obs = bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr
    L = len(lms)
    d_i, d_d, d_n = hipmem.DevBuf(L * 4), hipmem.DevBuf(L * 4), hipmem.DevBuf(4)
    st = hipmem.Stream()
    pn = N.ProjParams(*[getattr(pp, k) for k, _ in oracle.ProjParams._fields_])
    N.check(ex._h, ex._lib.hs_search_by_projection_device(ex._h, C.byref(Fg), C.c_void_p(bufs[4].ptr), L, C.byref(pn), C.c_void_p(d_i.ptr),
                                                          C.c_void_p(d_d.ptr), C.c_void_p(d_n.ptr), C.c_void_p(st.ptr)))
    st.synchronize()
    return d_i.to_numpy(np.int32, L), d_d.to_numpy(f32, L), int(d_n.to_numpy(np.int32, 1)[0])


def init_inputs(rng, fa):
    """frame-1 keypoints for SearchForInitialization: a shuffled subset of the frame's own, descriptors with a few bits flipped, previous
    positions jittered and partly on special values (NaN, inf, 1e10, the bounds)"""
    n = len(fa["kps"])
    n1 = min(n, 400)
    sel = rng.permutation(n)[:n1]
    k1 = fa["kps"][sel].copy()
    d1 = scenes.flip_bits(rng, fa["desc"][sel], rng.choice([0, 5, 30, 50, 51], n1))
    prev = np.stack([k1["x"], k1["y"]], 1).astype(f32)
    with np.errstate(all="ignore"):
        prev += rng.normal(0, 2, prev.shape).astype(f32)
    minx, maxx, miny, maxy = fa["bounds"]
    spec = np.array([np.nan, np.inf, -np.inf, 1e10, minx, maxx, miny, maxy], f32)
    hit = rng.random(prev.shape) < 0.05
    prev[hit] = spec[rng.integers(0, len(spec), hit.sum())]
    return k1, d1, prev


def check_case(m, case, rng, device_path=True):
    fa, s = case["fa"], case["sim3"]
    n = len(fa["kps"])
    Fo, ko = oracle.make_frame_view(oracle.FrameView, **fa)
    Fg, kg = oracle.make_frame_view(N.FrameView, **fa)
    with_ref = n <= PYREF_MAX_N and len(s["fb"]["kps"]) <= PYREF_MAX_N
    grid = pyref.AreaGrid(fa["kps"], fa["bounds"]) if with_ref else None
    tag = (case["kind"], n, len(case["lms"]))
    # hs_frame_grid
    want = oracle.frame_grid(Fo)
    assert np.array_equal(gpu_frame_grid(m, Fg), want), tag
    if with_ref:
        assert np.array_equal(grid.cells, want), tag
    # hs_search_by_projection_sim3
    gi, gt, gn = gpu_sim3_projection(m, Fg, case)
    oi, ot, on = oracle.search_by_projection_sim3(Fo, case["Scw"], case["lms"], case["th"], case["th_low"], case["kp_matched"])
    assert np.array_equal(gi, oi) and np.array_equal(gt, ot) and gn == on, tag + ("sim3 projection",)
    if with_ref:
        pi, pt, pn = pyref.search_by_projection_sim3(fa, case["Scw"], case["lms"], case["th"], case["th_low"], case["kp_matched"], grid=grid)
        assert np.array_equal(pi, oi) and np.array_equal(pt, ot) and pn == on, tag + ("pyref sim3 projection",)
    # hs_search_by_sim3
    F2o, k2o = oracle.make_frame_view(oracle.FrameView, **s["fb"])
    F2g, k2g = oracle.make_frame_view(N.FrameView, **s["fb"])
    gm, gn = gpu_sim3(m, Fg, F2g, s)
    om, on = oracle.search_by_sim3(Fo, s["lms1"], F2o, s["lms2"], s["s12"], s["R12"], s["t12"], s["th"], s["th_high"])
    assert np.array_equal(gm, om) and gn == on, tag + ("sim3",)
    if with_ref:
        pm, pn = pyref.search_by_sim3(fa, s["lms1"], s["fb"], s["lms2"], s["s12"], s["R12"], s["t12"], s["th"], s["th_high"],
                                      grids=(grid, pyref.AreaGrid(s["fb"]["kps"], s["fb"]["bounds"])))
        assert np.array_equal(pm, om) and pn == on, tag + ("pyref sim3",)
    # hs_search_by_projection: every preset of the mirror (host entry point), the local-map preset through _device
    th = float(case["th"])
    for name, call, pp in presets(m, th):
        gi, gd, gn = call(Fg, case["lms"])
        oi, od, on = oracle.search_by_projection(Fo, case["lms"], pp)
        assert np.array_equal(gi, oi) and np.array_equal(gd, od) and gn == on, tag + (name,)
        if name == "local map" and device_path and n > 0 and len(case["lms"]) > 0:
            di, dd, dn = gpu_projection_device(m, fa, case["lms"], pp)
            assert np.array_equal(di, oi) and np.array_equal(dd, od) and dn == on, tag + ("device",)
    # hs_search_for_initialization, window = the case's windowSize
    if n > 0:
        k1, d1, prev = init_inputs(rng, fa)
        fi = dict(fa, uR=None, kp_lm_obs=None, sensor=0)
        F2io, k3 = oracle.make_frame_view(oracle.FrameView, **fi)
        F2ig, k4 = oracle.make_frame_view(N.FrameView, **fi)
        gm, gprev, gn = m.SearchForInitialization(k1, d1, F2ig, prev, case["window"])
        om, oprev, on = oracle.search_for_initialization(k1, d1, F2io, prev, case["window"], m.TH_LOW, m.mfNNratio)
        assert np.array_equal(gm, om) and gn == on and np.array_equal(gprev.view(np.uint32), oprev.view(np.uint32)), tag + ("init", case["window"])


@pytest.mark.parametrize("block", range(3))
def test_area_edge_cases_all_entry_points(matcher, block):
    rng = np.random.default_rng(100 + block)
    for seed in range(200 + 8 * block, 200 + 8 * block + 8):
        for case in scenes.area_edge_cases(seed):
            check_case(matcher, case, rng)


def test_area_size_extremes_all_entry_points(matcher):
    """F.n of 0, 1 and 65 535, L of 0, 1, 64, 65 and 20 000, in an order that shrinks and grows the handle's scratch"""
    rng = np.random.default_rng(7)
    cases = list(scenes.area_size_cases(5))
    for i in (5, 0, 7, 1, 3, 6, 2, 4):
        check_case(matcher, cases[i], rng)


def test_out_of_range_radius_finds_nothing(matcher):
    """The radius th * size / size_ref at 3e10 or +inf: the reference's (int)ceil(...) is INT_MIN on x86-64, so the cell range is empty and no
    keypoint is a candidate; a NaN keypoint is outside the grid.  One keypoint at distance 0 sits right at the projection."""
    for size in (3e10 * 31, np.inf):
        d = np.zeros((2, 32), np.uint8)
        k = np.zeros(2, oracle.KP_DTYPE); k["x"], k["y"], k["size"] = (320.0, 100.0), (240.0, 100.0), (31.0, size)
        fa = dict(Rcw=np.eye(3, dtype=f32), tcw=np.zeros(3, f32), fx=512.0, fy=512.0, cx=320.0, cy=240.0, mbf=51.2, sensor=1,
                  bounds=(0.0, 640.0, 0.0, 480.0), kps=k, desc=d, uR=np.full(2, -1, f32), kp_lm_obs=np.full(2, -1, np.int32), size_ref=31.0)
        lm = np.zeros(2, oracle.LM_DTYPE)
        lm["pos"] = (0.0, 0.0, 2.0); lm["min_dist"], lm["max_dist"] = 1.0, 4.0; lm["normal"] = (0.0, 0.0, 1.0); lm["assoc_kp"] = (1, 0)
        Fg, kg = oracle.make_frame_view(N.FrameView, **fa)
        gi, gt, gn = gpu_sim3_projection(matcher, Fg, dict(lms=lm, Scw=np.eye(4, dtype=f32), th=1, th_low=50.0, kp_matched=np.zeros(2, np.uint8)))
        assert gi.tolist() == [-1, 0] and gn == 1, (size, gi)
        s = dict(lms1=lm, lms2=lm, s12=1.0, R12=np.eye(3, dtype=f32), t12=np.zeros(3, f32), th=1.0, th_high=100.0)
        gm, gn = gpu_sim3(matcher, Fg, Fg, s)
        assert gm.tolist() == [-1, -1] and gn == 0, (size, gm)                 # landmark 1 finds keypoint 0, whose own landmark finds nothing
    k = np.zeros(3, oracle.KP_DTYPE); k["x"], k["y"] = (np.nan, 1.0, 1e10), (1.0, np.nan, 1.0)
    Fg, kg = oracle.make_frame_view(N.FrameView, **dict(fa, kps=k, desc=np.zeros((3, 32), np.uint8), uR=None, kp_lm_obs=None))
    assert gpu_frame_grid(matcher, Fg).tolist() == [[-1, -1]] * 3


def test_known_image_bound_conventions(matcher):
    """u == max_x exactly (X/Z = 0.625, fx = 512, cx = 320): KeyFrame::IsInImage (strict) rejects the landmark in hs_search_by_projection_sim3,
    Camera::Project (inclusive) keeps it in hs_search_by_sim3 and hs_search_by_projection"""
    k = np.zeros(2, oracle.KP_DTYPE); k["x"], k["y"], k["size"] = (632.0, 634.0), (240.0, 240.0), 310.0      # radius 10 through assoc_kp
    fa = dict(Rcw=np.eye(3, dtype=f32), tcw=np.zeros(3, f32), fx=512.0, fy=512.0, cx=320.0, cy=240.0, mbf=51.2, sensor=1,
              bounds=(0.0, 640.0, 0.0, 480.0), kps=k, desc=np.zeros((2, 32), np.uint8), uR=np.full(2, -1, f32), kp_lm_obs=np.full(2, -1, np.int32), size_ref=31.0)
    lm = np.zeros(2, oracle.LM_DTYPE)
    lm["pos"] = (0.625, 0.0, 1.0); lm["normal"] = (0.53, 0.0, 0.848); lm["assoc_kp"] = 0
    lm["min_dist"], lm["max_dist"] = 0.5, 3.0
    Fg, kg = oracle.make_frame_view(N.FrameView, **fa)
    gi, gt, gn = gpu_sim3_projection(matcher, Fg, dict(lms=lm[:1], Scw=np.eye(4, dtype=f32), th=1, th_low=50.0, kp_matched=np.zeros(2, np.uint8)))
    assert gi.tolist() == [-1] and gn == 0
    s = dict(lms1=lm, lms2=lm, s12=1.0, R12=np.eye(3, dtype=f32), t12=np.zeros(3, f32), th=1.0, th_high=100.0)
    gm, gn = gpu_sim3(matcher, Fg, Fg, s)
    assert gm.tolist() == [0, -1] and gn == 1
    gi, gd, gn = matcher.SearchByProjectionKeyFrame(Fg, lm[:1], 1.0, 70)
    assert gi.tolist() == [0] and gn == 1


def test_published_frame_with_edge_landmarks(gpu):
    """hs_search_by_projection_frame: a published extraction, landmarks from the edge-case generator (sizes, radii, ties, bounds), each preset"""
    from hyslam_amd.synth import synth_stereo_pair
    Limg, Rimg = synth_stereo_pair(23, 640, 480)
    ex = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=1000))
    m = HS.FeatureMatcher(HS.FeatureMatcherSettings(nnratio=0.8), ex)
    (kl, _), (dl, _) = ex.extract_batch([Limg, Rimg], publish=True)
    rng = np.random.default_rng(11)
    n = len(kl)
    fa = dict(Rcw=np.eye(3, dtype=f32), tcw=np.zeros(3, f32), fx=512.0, fy=512.0, cx=320.0, cy=240.0, mbf=51.2, sensor=1, bounds=(0.0, 640.0, 0.0, 480.0),
              kps=kl, desc=dl, uR=(kl["x"] - rng.uniform(1, 40, n)).astype(f32), kp_lm_obs=rng.integers(-1, 3, n).astype(np.int32), size_ref=31.0)
    L = 3000
    lms = scenes._area_landmarks(rng, fa, rng.integers(0, n, L), rng.choice([0, 3, 20, 50, 90], L))
    a = rng.random(L) < 0.3
    lms["assoc_kp"][a] = rng.integers(0, n, a.sum())
    b = ~a & (rng.random(L) < 0.2)
    lms["size"][b] = rng.choice(np.array([0.0, 1e-40, 1e30, np.inf, -1.0, np.nan], f32), b.sum())
    scenes._landmark_edges(rng, {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in fa.items()}, lms, 3)   # the published frame stays as extracted
    Fo, ko = oracle.make_frame_view(oracle.FrameView, **fa)
    Fg, kg = oracle.make_frame_view(N.FrameView, **fa)
    for th in (0.0, 1.0, 5.0, 1e30):
        for name, call, pp in presets(m, th):
            gi, gd, gn = call(Fg, lms)
            assert m.frame_on_device, name
            oi, od, on = oracle.search_by_projection(Fo, lms, pp)
            assert np.array_equal(gi, oi) and np.array_equal(gd, od) and gn == on, (name, th)
    for t in ex.last_frame_tokens:
        ex.release_frame(t)
