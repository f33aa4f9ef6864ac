"""The stereo matcher's edge cases on every device entry point that takes keypoint lists (hs_stereo_match, hs_stereo_match_batch_device,
hs_stereo_match_frames) and the fused front end under varied matcher parameters: every result bit-identical to the CPU oracle and, wherever
it ran, to the numpy restatement pyref.stereo_match.  The lists come from scenes.stereo_edge_lists: rows on strip boundaries, outside
[0, n_rows) and bands over several strips, disparities at 0 and at maxD, octave steps of 1 and 2, equal distances in several strips,
distances at the thresholds and at the median cut, and list sizes past 2 048, 4 096 and up to 20 000."""
import numpy as np
import pytest

import hipmem
import oracle
import pyref
import scenes
import hyslam_amd as HS
from hyslam_amd import _native as N
from hyslam_amd.synth import synth_stereo_pair

pytestmark = pytest.mark.gpu
PYREF_MAX = 3000                      # the restatement runs on lists up to this size; beyond it the oracle alone is the reference


def expected(kL, dL, kR, dR, params):
    o = oracle.stereo_match(kL, dL, kR, dR, oracle.stereo_params(**params))
    if max(len(kL), len(kR)) <= PYREF_MAX:
        p = pyref.stereo_match(kL, dL, kR, dR, **params)
        assert np.array_equal(o[0], p[0]) and np.array_equal(o[1], p[1]), "oracle and pyref disagree: %r" % (params,)
    return o


def assert_parity(u, z, ref, what):
    ou, oz, obi, obd = ref
    bad = np.nonzero((u.view(np.uint32) != ou.view(np.uint32)) | (z.view(np.uint32) != oz.view(np.uint32)))[0]
    assert len(bad) == 0, "%s: %d of %d keypoints differ; first iL=%d: device (uR %r, depth %r), oracle (uR %r, depth %r, best iR %d at distance %d)" % (
        what, len(bad), len(u), bad[0], u[bad[0]], z[bad[0]], ou[bad[0]], oz[bad[0]], obi[bad[0]], obd[bad[0]])


def host_call(ex, kL, dL, kR, dR, params):
    cam = HS.Camera(params["fx"], params["mbf"], float(params["n_rows"]))
    sm = HS.Stereomatcher(kL, kR, dL, dR, cam, settings=HS.FeatureMatcherSettings(TH_HIGH=params["th_high"], TH_LOW=params["th_low"]),
                          extractor=ex, size_ref=params["size_ref"])
    sm.computeStereoMatches()
    assert not sm.frames_on_device
    return sm.getData()


@pytest.fixture(scope="module")
def ex():
    return HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=1000))


@pytest.mark.parametrize("kind", scenes.STEREO_EDGE_KINDS)
def test_host_entry_point_edge_cases(gpu, ex, kind):
    """hs_stereo_match: generated cases of one kind over n_rows, band widths and thresholds (one pair: k_stereo_match<1>)"""
    rng = np.random.default_rng(1000 + sum(map(ord, kind)))
    for case in range(16):
        kL, dL, kR, dR, params = scenes.stereo_edge_lists(rng, kind, th=(80.0, 120.0) if case == 15 else None)
        u, z = host_call(ex, kL, dL, kR, dR, params)
        assert_parity(u, z, expected(kL, dL, kR, dR, params), "%s case %d %r" % (kind, case, params))


@pytest.mark.parametrize("n_rows", [0, 1, 33, 480, 1080, 1087])
def test_host_entry_point_parameter_grid(gpu, ex, n_rows):
    rng = np.random.default_rng(2000 + n_rows)
    for size_ref in (31.0, 7.5, 4.0, 1e6):
        for th in scenes.STEREO_THRESHOLDS + ((80.0, 120.0), (80.5, 100.0)):
            kind = scenes.STEREO_EDGE_KINDS[int(rng.integers(len(scenes.STEREO_EDGE_KINDS)))]
            kL, dL, kR, dR, params = scenes.stereo_edge_lists(rng, kind, n_rows=n_rows, size_ref=size_ref, th=th)
            u, z = host_call(ex, kL, dL, kR, dR, params)
            assert_parity(u, z, expected(kL, dL, kR, dR, params), repr(params))
            if n_rows == 0:
                assert (u == -1).all() and (z == -1).all()


@pytest.mark.parametrize("nL,nR", [(0, 5), (1, 0), (1, 1), (7, 0), (2049, 2049), (2999, 700), (4097, 4097), (9000, 3000), (9000, 9000),
                                   (20000, 20000)])
def test_host_entry_point_list_sizes(gpu, ex, nL, nR):
    """past 2 048 left keypoints the median kernel reads the distances in a loop, past 4 096 right keypoints the strip kernel loops,
    from 16 384 the single pair runs k_stereo_match<2>"""
    rng = np.random.default_rng(nL * 7 + nR)
    for kind, kw in (("mixed", dict(size_ref=7.5)), ("median", {}), ("boundaries", dict(size_ref=4.0)), ("thresholds", dict(th=(257.0, 256.0)))):
        kL, dL, kR, dR, params = scenes.stereo_edge_lists(rng, kind, nL=nL, nR=nR, n_rows=1087, **kw)
        u, z = host_call(ex, kL, dL, kR, dR, params)
        ref = expected(kL, dL, kR, dR, params)
        assert_parity(u, z, ref, "%s %d x %d %r" % (kind, nL, nR, params))
        if nL > 1000 and nR > 1000:
            assert (ref[1] > 0).sum() > nL // 50


def run_batch(ex, cases, cap, params):
    """hs_stereo_match_batch_device on `cases` [(kL, dL, kR, dR)] laid out with stride cap; every pair against the oracle"""
    P = len(cases)
    kL, kR = np.zeros((P, cap), N.KP_DTYPE), np.zeros((P, cap), N.KP_DTYPE)
    dL, dR = np.zeros((P, cap, 32), np.uint8), np.zeros((P, cap, 32), np.uint8)
    nL, nR = np.zeros(P, np.int32), np.zeros(P, np.int32)
    for j, (a, b, c, d) in enumerate(cases):
        nL[j], nR[j] = len(a), len(c)
        kL[j, :len(a)], dL[j, :len(a)], kR[j, :len(c)], dR[j, :len(c)] = a, b, c, d
    bufs = [hipmem.DevBuf.from_numpy(x) for x in (kL, dL, nL, kR, dR, nR)]
    d_u, d_z = hipmem.DevBuf(P * cap * 4), hipmem.DevBuf(P * cap * 4)
    sp = N.StereoParams(params["fx"], params["mbf"], params["n_rows"], params["th_high"], params["th_low"], params["size_ref"])
    ex.stereo_match_batch_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, P, cap, sp, d_u.ptr, d_z.ptr, 0)
    ex.synchronize()
    u, z = d_u.to_numpy(np.float32, P * cap).reshape(P, cap), d_z.to_numpy(np.float32, P * cap).reshape(P, cap)
    for j, (a, b, c, d) in enumerate(cases):
        assert_parity(u[j, :nL[j]], z[j, :nL[j]], expected(a, b, c, d, params), "pair %d of %d (nL %d, nR %d), cap %d, %r" % (j, P, nL[j], nR[j], cap, params))


def batch_cases(rng, sizes, params):
    out = []
    for j, (nl, nr) in enumerate(sizes):
        kind = scenes.STEREO_EDGE_KINDS[j % len(scenes.STEREO_EDGE_KINDS)]
        kL, dL, kR, dR, _ = scenes.stereo_edge_lists(rng, kind, nL=nl, nR=nr, n_rows=params["n_rows"], size_ref=params["size_ref"],
                                                     th=(params["th_high"], params["th_low"]), fx=params["fx"])
        out.append((kL, dL, kR, dR))
    return out


def test_batch_device_both_matchers_and_scratch_reuse(gpu):
    """pairs * cap below 16 384 runs k_stereo_match<1>, from 16 384 on k_stereo_match<2> (8 x 2048 is the first, 7 x 2339 the last below);
    odd caps and counts; pairs of very different sizes in one batch; one handle first with a large n_rows and cap, then with more pairs at
    a smaller cap and n_rows (strip counters grow, strip lists do not), then larger again"""
    ex = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=1000))
    rng = np.random.default_rng(77)
    runs = [
        (dict(fx=500.0, mbf=60.0, n_rows=1087, th_high=100.0, th_low=51.0, size_ref=7.5), 4097, [(4097, 4097), (0, 300), (1, 4000), (3001, 17), (999, 2500)]),
        (dict(fx=500.0, mbf=60.0, n_rows=480, th_high=80.0, th_low=45.0, size_ref=4.0), 301, [(301, 301), (17, 300), (0, 0), (150, 1)] * 12),
        (dict(fx=5.25, mbf=0.63, n_rows=33, th_high=257.0, th_low=256.0, size_ref=31.0), 1001, [(1001, 999), (3, 1001), (500, 500)]),
        (dict(fx=1050.0, mbf=126.0, n_rows=1080, th_high=100.0, th_low=50.0, size_ref=31.0), 2048, [(2048, 2048), (1, 2047), (2047, 1), (1023, 1999)] * 2),
        (dict(fx=1050.0, mbf=126.0, n_rows=1087, th_high=100.0, th_low=51.0, size_ref=4.0), 2339, [(2339, 2339), (1, 2339), (2339, 1), (1023, 1999)] + [(2049, 2339)] * 3),
        (dict(fx=500.0, mbf=250.0, n_rows=1080, th_high=80.0, th_low=120.0, size_ref=7.5), 1999, [(1999, 1999), (1500, 700), (3, 1999)] * 3),
        (dict(fx=1e5, mbf=7000.0, n_rows=1087, th_high=100.0, th_low=50.0, size_ref=1e6), 9000, [(9000, 9000), (4500, 8999)]),
    ]
    for params, cap, sizes in runs:
        run_batch(ex, batch_cases(rng, sizes, params), cap, params)


def test_device_resident_frames_with_matcher_parameters(gpu):
    """hs_stereo_match_frames: both views published by the extractor, the matcher run on the device copies with other parameters"""
    L, R = synth_stereo_pair(61, 640, 480)
    ex = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=2000))
    (kl, kr), (dl, dr) = ex.extract_batch([L, R], publish=True)
    tl, tr = ex.last_frame_tokens
    try:
        for fx, mbf, n_rows, th, size_ref in ((500.0, 60.0, 480, (100.0, 50.0), 31.0), (500.0, 60.0, 300, (80.0, 45.0), 7.5),
                                             (500.0, 60.0, 33, (100.0, 51.0), 4.0), (500.0, 60.0, 480, (257.0, 256.0), 4.0),
                                             (5.0, 0.6, 480, (80.0, 120.0), 1e6), (500.0, 60.0, 0, (100.0, 50.0), 31.0)):
            params = dict(fx=fx, mbf=mbf, n_rows=n_rows, th_high=th[0], th_low=th[1], size_ref=size_ref)
            cam = HS.Camera(fx, mbf, float(n_rows))
            sm = HS.Stereomatcher(kl, kr, dl, dr, cam, settings=HS.FeatureMatcherSettings(TH_HIGH=th[0], TH_LOW=th[1]), extractor=ex, size_ref=size_ref)
            sm.computeStereoMatches()
            assert sm.frames_on_device, params
            u, z = sm.getData()
            assert_parity(u, z, expected(kl, dl, kr, dr, params), "frames %r" % (params,))
    finally:
        ex.release_frame(tl)
        ex.release_frame(tr)


FRONTEND_PARAMS = [(31.0, (100.0, 50.0), 480), (7.5, (80.0, 45.0), 480), (4.0, (100.0, 51.0), 300), (4.0, (257.0, 256.0), 33),
                   (31.0, (80.0, 120.0), 480), (7.5, (100.0, 50.0), 0)]


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_fused_front_end_with_matcher_parameters(gpu, fuse, monkeypatch):
    """hs_stereo_frontend_batch_device (strips binned in the describe launch with HS_STEREO_FUSE=1, by k_stereo_strips with 0) and
    submit_batch with a StereoParams: extractor keypoints, matcher parameters varied; against oracle.stereo_frontend and against pyref on
    the device's own keypoints"""
    monkeypatch.setenv("HS_STEREO_FUSE", fuse)                   # read when the handle is created
    W, H, P, NF = 640, 480, 3, 2000
    ex = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=NF))
    p = oracle.default_params(NF)
    pairs = [synth_stereo_pair(500 + i, W, H) for i in range(P)]
    left = np.stack([a for a, _ in pairs]); right = np.stack([b for _, b in pairs])
    ex.reserve(W, H, 2 * P)
    cap = ex.max_keypoints()
    dl, dr = hipmem.DevBuf.from_numpy(left), hipmem.DevBuf.from_numpy(right)
    dk = [hipmem.DevBuf(P * cap * N.KP_DTYPE.itemsize) for _ in range(2)]; dd = [hipmem.DevBuf(P * cap * 32) for _ in range(2)]
    dn = [hipmem.DevBuf(P * 4) for _ in range(2)]
    du, dz = hipmem.DevBuf(P * cap * 4), hipmem.DevBuf(P * cap * 4)
    pin = ex.pinned_frames(2 * P, H, W)
    for i in range(P):
        pin[i], pin[P + i] = pairs[i]
    for size_ref, th, n_rows in FRONTEND_PARAMS:
        params = dict(fx=500.0, mbf=60.0, n_rows=n_rows, th_high=th[0], th_low=th[1], size_ref=size_ref)
        sp = N.StereoParams(500.0, 60.0, n_rows, th[0], th[1], size_ref)
        osp = oracle.stereo_params(**params)
        ref = [oracle.stereo_frontend(p, osp, L, R) for L, R in pairs]
        ex.stereo_frontend_batch_device(dl.ptr, dr.ptr, P, W, H, W, W * H, dk[0].ptr, dd[0].ptr, dn[0].ptr, dk[1].ptr, dd[1].ptr, dn[1].ptr,
                                        cap, sp, du.ptr, dz.ptr, 0)
        ex.synchronize()
        nL, nR = dn[0].to_numpy(np.int32, P), dn[1].to_numpy(np.int32, P)
        kL = dk[0].to_numpy(N.KP_DTYPE, P * cap).reshape(P, cap); kR = dk[1].to_numpy(N.KP_DTYPE, P * cap).reshape(P, cap)
        dL = dd[0].to_numpy(np.uint8, P * cap * 32).reshape(P, cap, 32); dR = dd[1].to_numpy(np.uint8, P * cap * 32).reshape(P, cap, 32)
        u, z = du.to_numpy(np.float32, P * cap).reshape(P, cap), dz.to_numpy(np.float32, P * cap).reshape(P, cap)
        n, k, d, tu, tz = ex.wait(ex.submit_batch([pin[i] for i in range(2 * P)], sp))
        for i, (okL, odL, okR, odR, ou, oz) in enumerate(ref):
            what = "pair %d, fuse %s, %r" % (i, fuse, params)
            assert nL[i] == len(okL) and nR[i] == len(okR), what
            assert kL[i, :nL[i]].tobytes() == okL.tobytes() and kR[i, :nR[i]].tobytes() == okR.tobytes(), what
            assert np.array_equal(dL[i, :nL[i]], odL) and np.array_equal(dR[i, :nR[i]], odR), what
            gk, gd, gkr, gdr = kL[i, :nL[i]], dL[i, :nL[i]], kR[i, :nR[i]], dR[i, :nR[i]]
            ref_i = oracle.stereo_match(gk, gd, gkr, gdr, osp)
            assert np.array_equal(ref_i[0], ou) and np.array_equal(ref_i[1], oz), what
            pu, pz, _, _ = pyref.stereo_match(gk, gd, gkr, gdr, **params)
            assert np.array_equal(pu, ou) and np.array_equal(pz, oz), "pyref on the device's keypoints: " + what
            assert_parity(u[i, :nL[i]], z[i, :nL[i]], ref_i, "front end " + what)
            assert n[i] == nL[i] and n[P + i] == nR[i] and k[i, :n[i]].tobytes() == okL.tobytes(), what
            assert_parity(tu[i, :n[i]], tz[i, :n[i]], ref_i, "submit_batch " + what)
            if n_rows == 0:
                assert (oz == -1).all()
