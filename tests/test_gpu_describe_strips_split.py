"""The stereo strip builder — the extra workgroup of the front end's describe launch, which shares the kernel with the keypoint waves — must fill
exactly what k_stereo_match reads, whatever is done to keep it out of the keypoint path's way (kernels_describe.hip: describe_strips_block).

One call of hs_stereo_frontend_batch_device on 160 x 120 frames (four 32-row strips, the last one 24 rows): a noise pair whose right keypoints lie
in the first and in the last strip as well as in between, and the same left frame with a flat right frame — no right keypoint at all, so every strip
of that pair must come out empty.  Keypoints, descriptors, uRight and depth of both pairs against oracle.stereo_frontend; twice on the same
handle with the outputs overwritten in between (nothing may be left over from the first call)."""
import numpy as np
import pytest

import hipmem
import oracle
import hyslam_amd as HS
from hyslam_amd import _native as N

pytestmark = pytest.mark.gpu
W, H, NF = 160, 120, 500


def scene():
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (H, W + 16), dtype=np.uint8)
    left, right = base[:, 8:8 + W].copy(), base[:, 12:12 + W].copy()      # the right view: the left one 4 px further left
    return [(left, right), (left, np.full((H, W), 90, np.uint8))]


def test_strips_of_first_and_last_rows_and_of_an_empty_right_image(gpu):
    pairs = scene()
    P = len(pairs)
    p = oracle.default_params(NF)
    params = dict(fx=200.0, mbf=24.0, n_rows=H)
    osp = oracle.stereo_params(**params)
    ref = [oracle.stereo_frontend(p, osp, L, R) for L, R in pairs]
    yR = ref[0][2]["y"]
    assert (yR < 32).sum() > 0 and (yR >= 96).sum() > 0 and ((yR >= 32) & (yR < 96)).sum() > 0      # first, last and inner strips are all in use
    assert len(ref[0][0]) > 100 and (ref[0][5] > 0).sum() > 20                                       # ... and the pair really matches
    assert len(ref[1][2]) == 0 and len(ref[1][0]) == len(ref[0][0]) and (ref[1][5] <= 0).all()       # no right keypoint: no match

    ex = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=NF))
    ex.reserve(W, H, 2 * P)
    cap = ex.max_keypoints()
    sp = N.StereoParams(params["fx"], params["mbf"], H, 100.0, 50.0, 31.0)
    dl = hipmem.DevBuf.from_numpy(np.stack([a for a, _ in pairs]))
    dr = hipmem.DevBuf.from_numpy(np.stack([b for _, b in pairs]))
    dk = [hipmem.DevBuf(P * cap * N.KP_DTYPE.itemsize) for _ in range(2)]
    dd = [hipmem.DevBuf(P * cap * 32) for _ in range(2)]
    dn = [hipmem.DevBuf(P * 4) for _ in range(2)]
    du, dz = hipmem.DevBuf(P * cap * 4), hipmem.DevBuf(P * cap * 4)
    for rep in range(2):
        for b in dk + dd + dn + [du, dz]:
            b.fill(0xA5)
        ex.stereo_frontend_batch_device(dl.ptr, dr.ptr, P, W, H, W, W * H, dk[0].ptr, dd[0].ptr, dn[0].ptr, dk[1].ptr, dd[1].ptr, dn[1].ptr,
                                        cap, sp, du.ptr, dz.ptr, 0)
        ex.synchronize()
        nL, nR = dn[0].to_numpy(np.int32, P), dn[1].to_numpy(np.int32, P)
        kL = dk[0].to_numpy(N.KP_DTYPE, P * cap).reshape(P, cap); kR = dk[1].to_numpy(N.KP_DTYPE, P * cap).reshape(P, cap)
        dL = dd[0].to_numpy(np.uint8, P * cap * 32).reshape(P, cap, 32); dR = dd[1].to_numpy(np.uint8, P * cap * 32).reshape(P, cap, 32)
        u, z = du.to_numpy(np.float32, P * cap).reshape(P, cap), dz.to_numpy(np.float32, P * cap).reshape(P, cap)
        for i, (okL, odL, okR, odR, ou, oz) in enumerate(ref):
            what = "call %d, pair %d" % (rep, i)
            assert nL[i] == len(okL) and nR[i] == len(okR), (what, nL[i], len(okL), nR[i], len(okR))
            assert kL[i, :nL[i]].tobytes() == okL.tobytes() and kR[i, :nR[i]].tobytes() == okR.tobytes(), what
            assert np.array_equal(dL[i, :nL[i]], odL) and np.array_equal(dR[i, :nR[i]], odR), what
            bad = np.nonzero((u[i, :nL[i]].view(np.uint32) != ou.view(np.uint32)) | (z[i, :nL[i]].view(np.uint32) != oz.view(np.uint32)))[0]
            assert len(bad) == 0, "%s: %d of %d left keypoints differ, first %d: device (uR %r, depth %r), oracle (%r, %r)" % (
                what, len(bad), nL[i], bad[0], u[i, bad[0]], z[i, bad[0]], ou[bad[0]], oz[bad[0]])
