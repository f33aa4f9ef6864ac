"""The HIP extractor against the independent numpy restatement of the whole extractor (tests/ref_extract.py) on the directed scenes of
tests/extract_cases.py: cell-loop geometry, levels without cells, retried cells, cell seams, all-equal responses, axis angles, the ends of the byte
range, the quota arithmetic and the front ends.  Every expected value comes from ref_extract, never from the oracle; every comparison is bit-exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

import extract_cases as X
import hipmem
import ref_extract as R
import hyslam_amd as HS
from hyslam_amd import _native as N
from _extract_edge_check import assert_features, check_case, make_extractor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KB = N.KP_DTYPE.itemsize


@pytest.mark.parametrize("name", list(X.CASES))
def test_case_stagewise(gpu, name):
    check_case(name)


def test_batch_of_mixed_content(gpu):
    """one extract_batch of equal-sized frames, the tie-heavy periodic frame between ordinary ones: nothing leaks from a frame to its neighbours;
    then the same frames in another order and the periodic frame three times over on the same handle"""
    ex = make_extractor(**X.GEOM)
    for order in (X.BATCH_273x225, X.BATCH_273x225[::-1], ["periodic_seams"] * 3 + ["geom_273x225"]):
        ks, ds = ex.extract_batch([X.CASES[n]["img"] for n in order])
        for n, gk, gd in zip(order, ks, ds):
            assert_features(n, gk, gd, *X.reference(n)[:2])
    ex2 = make_extractor(**X.settings_of(X.CASES["periodic_ties"]))
    ks, ds = ex2.extract_batch([X.CASES[n]["img"] for n in ("retry_low_contrast", "periodic_ties", "byte_range_t20", "periodic_ties")])
    for i in (1, 3):                                             # (the other two frames run at another quota than their case's: only the tie frame is compared)
        assert_features("periodic_ties", ks[i], ds[i], *X.reference("periodic_ties")[:2])


def test_device_batch_with_a_row_stride_above_the_width(gpu):
    names = X.BATCH_273x225
    B, W, H, S = len(names), 273, 225, 320
    frames = np.full((B, H, S), 0xA5, np.uint8)                  # the padding is not black: reading past the width would show
    for i, n in enumerate(names):
        frames[i, :, :W] = X.CASES[n]["img"]
    ex = make_extractor(**X.GEOM)
    ex.reserve(W, H, B)
    cap = ex.max_keypoints()
    d_img = hipmem.DevBuf.from_numpy(frames)
    d_k, d_d, d_n = hipmem.DevBuf(B * cap * KB), hipmem.DevBuf(B * cap * 32), hipmem.DevBuf(B * 4)
    ex.extract_batch_device(d_img.ptr, B, W, H, S, S * H, d_k.ptr, d_d.ptr, d_n.ptr, cap, 0)
    ex.synchronize()
    n = d_n.to_numpy(np.int32, B)
    kps = d_k.to_numpy(N.KP_DTYPE, B * cap).reshape(B, cap)
    desc = d_d.to_numpy(np.uint8, B * cap * 32).reshape(B, cap, 32)
    for i, name in enumerate(names):
        assert_features(name, kps[i, :n[i]], desc[i, :n[i]], *X.reference(name)[:2])


@pytest.mark.parametrize("scale", X.QUOTA_SCALES)
def test_tables_over_the_quota_grid(gpu, scale):
    """GetFeaturesPerLevel, GetScaleFactors and hs_orb_get_scale_tables == ref_extract.tables.  A level quota above 3320 is refused at create with a
    status (test_gpu_parity.py::test_quota_beyond_the_large_instance_is_refused_cleanly); nothing else in the grid may be refused."""
    refused = 0
    for L in X.QUOTA_LEVELS:
        for nf in X.QUOTA_NFEATURES:
            ref = R.tables(nf, scale, L)
            st = HS.FeatureExtractorSettings(nFeatures=nf, fScaleFactor=scale, nLevels=L)
            if int(ref[4].max()) > 3320:
                with pytest.raises(HS.HsError) as e:
                    HS.ORBExtractor(st)
                assert e.value.status == N.HS_ERR_INVALID, (nf, scale, L)
                refused += 1
                continue
            ex = HS.ORBExtractor(st)
            assert ex.GetLevels() == L
            for a, b in zip(ref, ex._tables()):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (nf, scale, L)
            if nf in (1, 1000, 15000):
                assert ex.GetFeaturesPerLevel().tobytes() == ref[4].tobytes() and ex.GetScaleFactors().tobytes() == ref[0].tobytes()
                assert ex.GetInverseScaleFactors().tobytes() == ref[1].tobytes() and ex.GetScaleSigmaSquares().tobytes() == ref[2].tobytes()
                assert ex.GetInverseScaleSigmaSquares().tobytes() == ref[3].tobytes()
            ex.close()
    assert refused > 0                                           # 15000 features on one or two levels


def test_stereo_front_end_two_pairs_on_the_device(gpu):
    """hs_stereo_frontend_batch_device on two small pairs == ref_extract.stereo_frontend (extract twice + pyref.stereo_match)"""
    kw = X.STEREO
    pairs = X.stereo_pairs()
    P, W, H = len(pairs), 320, 240
    ex = make_extractor(kw["nfeatures"], kw["scale"], kw["nlevels"], kw["n_cells"])
    ex.reserve(W, H, 2 * P)
    cap = ex.max_keypoints()
    dl, dr = hipmem.DevBuf.from_numpy(np.stack([a for a, _ in pairs])), hipmem.DevBuf.from_numpy(np.stack([b for _, b in pairs]))
    dk = [hipmem.DevBuf(P * cap * KB) for _ in range(2)]
    dd = [hipmem.DevBuf(P * cap * 32) for _ in range(2)]
    dn = [hipmem.DevBuf(P * 4) for _ in range(2)]
    du, dz = hipmem.DevBuf(P * cap * 4), hipmem.DevBuf(P * cap * 4)
    sp = N.StereoParams(kw["fx"], kw["mbf"], kw["n_rows"], 100.0, 50.0, 31.0)
    ex.stereo_frontend_batch_device(dl.ptr, dr.ptr, P, W, H, W, W * H, dk[0].ptr, dd[0].ptr, dn[0].ptr, dk[1].ptr, dd[1].ptr, dn[1].ptr, cap, sp, du.ptr, dz.ptr, 0)
    ex.synchronize()
    nL, nR = dn[0].to_numpy(np.int32, P), dn[1].to_numpy(np.int32, P)
    kL, kR = (b.to_numpy(N.KP_DTYPE, P * cap).reshape(P, cap) for b in dk)
    dL, dR = (b.to_numpy(np.uint8, P * cap * 32).reshape(P, cap, 32) for b in dd)
    u, z = du.to_numpy(np.float32, P * cap).reshape(P, cap), dz.to_numpy(np.float32, P * cap).reshape(P, cap)
    for i in range(P):
        rkL, rdL, rkR, rdR, ru, rz = X.stereo_reference(i)
        assert int((rz > 0).sum()) > 30
        assert_features("left %d" % i, kL[i, :nL[i]], dL[i, :nL[i]], rkL, rdL)
        assert_features("right %d" % i, kR[i, :nR[i]], dR[i, :nR[i]], rkR, rdR)
        assert u[i, :nL[i]].tobytes() == ru.tobytes() and z[i, :nL[i]].tobytes() == rz.tobytes(), i


@pytest.mark.parametrize("scale", X.CAMERA_SCALES)
def test_camera_frame_front_end(gpu, scale):
    """extract_camera_batch on a BGR frame (0.5: the 2 x 2 area path; 0.75: bilinear) == pyref.preprocess + ref_extract.extract"""
    kw = X.CAMERA
    ex = make_extractor(kw["nfeatures"], kw["scale"], kw["nlevels"], kw["n_cells"])
    ks, ds, greys = ex.extract_camera_batch([X.colour_frame(71)], False, scale, want_grey=True)
    grey, rk, rd = X.camera_reference(scale)
    assert np.array_equal(greys[0], grey)
    assert_features("camera %g" % scale, ks[0], ds[0], rk, rd)


@pytest.mark.parametrize("env", [{"HS_FAST_COLS": "32"}, {"HS_FAST_KEYS": "0"}, {"HS_QT_POINT_DOMAIN": "1"}])
def test_kernel_variants_in_subprocess(gpu, env):
    """the narrow FAST work items, the quadtree gathering candidates and computing their keys itself, and its point-domain passes, each in a fresh
    child process, on the seam, tie, cell-edge and retry cases and the mixed batch"""
    e = dict(os.environ)
    e.update(env)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_extract_edge_check.py")], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "EXTRACT_EDGES_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
