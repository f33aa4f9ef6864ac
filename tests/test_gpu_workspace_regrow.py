"""GPU: ONE handle walks its owned workspace buffers through grow, reuse-smaller and grow-again, and a batch through the odd two-lane split,
every result bit-exact against the CPU oracle.  The sequence: a host extraction of one small frame (first allocations); two stereo tickets of a
larger frame in flight, waited for in reverse order (both ingest slots and the stereo buffers grow, the geometry is rebuilt); camera frames
that land on the FIRST geometry with a larger batch (the geometry and the result block grow again, the raw staging is allocated, the grey
frames come back); hs_stereo_match at (1, 0), (600, 700) and (1, 1) keypoints (its staging: first allocation, regrow, reuse); the first call
again (every buffer is now larger than it needs); the device front ends on two lanes with 3 items (split 1 + 2) and 1 item (no split); a
mono ticket (a result block without uRight / depth in a slot that held a stereo one); and the first call once more."""
import numpy as np
import pytest

import hipmem
import oracle
import hyslam_amd as HS
from hyslam_amd import _native as N
from hyslam_amd.synth import synth_image, synth_stereo_pair

pytestmark = pytest.mark.gpu

NF = 1000
W0, H0 = 320, 240
W1, H1 = 640, 480


def same_features(k, d, ok, od):
    return len(k) == len(ok) and k.tobytes() == ok.tobytes() and np.array_equal(d, od)


def test_one_handle_grows_reuses_and_splits(gpu):
    ex = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=NF))
    p = oracle.default_params(NF)
    small = synth_image(11, W0, H0)
    ok0, od0 = oracle.extract(p, small)
    assert len(ok0) > 200

    def first_call_again(what):
        k, d = ex.extract_batch([small])
        assert same_features(k[0], d[0], ok0, od0), what

    # 1. host extract_batch, 1 frame, 320 x 240
    first_call_again("first call")

    # 2. two stereo tickets in flight, 2 frames each, 640 x 480, waited for in reverse order
    sp = HS.stereo_params(HS.Camera(fx=500.0, mbf=60.0, mnMaxY=float(H1)))
    osp = oracle.stereo_params(fx=500.0, mbf=60.0, n_rows=H1)
    big = [synth_stereo_pair(40 + i, W1, H1) for i in range(2)]
    tickets = [ex.submit_batch(list(pair), sp) for pair in big]
    ref_big = [oracle.stereo_frontend(p, osp, L, R) for L, R in big]
    for j in (1, 0):
        n, k, d, u, z = ex.wait(tickets[j])
        okL, odL, okR, odR, ou, oz = ref_big[j]
        assert same_features(k[0, :n[0]], d[0, :n[0]], okL, odL) and same_features(k[1, :n[1]], d[1, :n[1]], okR, odR), j
        assert np.array_equal(u[0, :n[0]].view(np.uint32), ou.view(np.uint32)) and np.array_equal(z[0, :n[0]].view(np.uint32), oz.view(np.uint32)), j
        assert (oz > 0).sum() > 50

    # 3. extract_camera_batch, 3 frames of 3 channels, 640 x 480 at scale 0.5: step 1's level-0 size with a larger batch; the grey frames come back
    colour = [np.ascontiguousarray(np.stack([synth_image(60 + 10 * i + 7 * c, W1, H1) for c in range(3)], axis=2)) for i in range(3)]
    k, d, grey = ex.extract_camera_batch(colour, True, 0.5, want_grey=True)
    for i, f in enumerate(colour):
        og = oracle.preprocess(f, True, 0.5)
        assert og.shape == (H0, W0) and np.array_equal(grey[i], og), i
        ok, od = oracle.extract(p, og)
        assert len(ok) > 200 and same_features(k[i], d[i], ok, od), i

    # 4. hs_stereo_match with (nL, nR) = (1, 0), (600, 700), (1, 1): keypoints of step 2's first pair
    okL, odL, okR, odR = ref_big[0][:4]
    assert len(okL) >= 600 and len(okR) >= 700
    cam = HS.Camera(500.0, 60.0, float(H1))
    for nL, nR in ((1, 0), (600, 700), (1, 1)):
        kL, dL, kR, dR = okL[:nL], odL[:nL], okR[:nR], odR[:nR]
        sm = HS.Stereomatcher(kL, kR, dL, dR, cam, extractor=ex)
        sm.computeStereoMatches()
        assert not sm.frames_on_device
        u, z = sm.getData()
        ou, oz, _, _ = oracle.stereo_match(kL, dL, kR, dR, osp)
        assert np.array_equal(u.view(np.uint32), ou.view(np.uint32)) and np.array_equal(z.view(np.uint32), oz.view(np.uint32)), (nL, nR)
        if nL == 600:
            assert (oz > 0).sum() > 50

    # 5. step 1 again
    first_call_again("after the larger calls")

    # 6. two lanes: the stereo front end with 3 pairs (split 1 + 2) and with 1 pair (no split), 320 x 240; extract_batch_device with 3 frames
    P = 3
    pairs = [synth_stereo_pair(80 + i, W0, H0) for i in range(P)]
    sp0 = HS.stereo_params(HS.Camera(fx=250.0, mbf=30.0, mnMaxY=float(H0)))
    osp0 = oracle.stereo_params(fx=250.0, mbf=30.0, n_rows=H0)
    ref = [oracle.stereo_frontend(p, osp0, L, R) for L, R in pairs]
    ex.set_lanes(2)
    ex.reserve(W0, H0, 2 * P)
    cap = ex.max_keypoints()
    dl, dr = hipmem.DevBuf.from_numpy(np.stack([a for a, _ in pairs])), hipmem.DevBuf.from_numpy(np.stack([b for _, b in pairs]))
    dk = [hipmem.DevBuf(P * cap * N.KP_DTYPE.itemsize) for _ in range(2)]; dd = [hipmem.DevBuf(P * cap * 32) for _ in range(2)]
    dn = [hipmem.DevBuf(P * 4) for _ in range(2)]
    du, dz = hipmem.DevBuf(P * cap * 4), hipmem.DevBuf(P * cap * 4)

    def read(npairs):
        ex.synchronize()
        n = [b.to_numpy(np.int32, npairs) for b in dn]
        k = [b.to_numpy(N.KP_DTYPE, npairs * cap).reshape(npairs, cap) for b in dk]
        d = [b.to_numpy(np.uint8, npairs * cap * 32).reshape(npairs, cap, 32) for b in dd]
        return n, k, d, du.to_numpy(np.float32, npairs * cap).reshape(npairs, cap), dz.to_numpy(np.float32, npairs * cap).reshape(npairs, cap)

    for npairs in (3, 1):
        for b in dn + [du, dz]:
            b.fill(0xEE)
        ex.stereo_frontend_batch_device(dl.ptr, dr.ptr, npairs, W0, H0, W0, W0 * H0, dk[0].ptr, dd[0].ptr, dn[0].ptr, dk[1].ptr, dd[1].ptr, dn[1].ptr,
                                        cap, sp0, du.ptr, dz.ptr, 0)
        n, k, d, u, z = read(npairs)
        for i in range(npairs):
            okL, odL, okR, odR, ou, oz = ref[i]
            what = (npairs, i)
            assert same_features(k[0][i, :n[0][i]], d[0][i, :n[0][i]], okL, odL) and same_features(k[1][i, :n[1][i]], d[1][i, :n[1][i]], okR, odR), what
            assert np.array_equal(u[i, :n[0][i]].view(np.uint32), ou.view(np.uint32)) and np.array_equal(z[i, :n[0][i]].view(np.uint32), oz.view(np.uint32)), what
    dn[0].fill(0xEE)
    ex.extract_batch_device(dl.ptr, P, W0, H0, W0, W0 * H0, dk[0].ptr, dd[0].ptr, dn[0].ptr, cap, 0)
    n, k, d, _, _ = read(P)
    for i in range(P):
        assert same_features(k[0][i, :n[0][i]], d[0][i, :n[0][i]], ref[i][0], ref[i][1]), i
    ex.set_lanes(1)

    # 7. one mono ticket at 320 x 240, then the handle still serves step 1
    n, k, d, u, z = ex.wait(ex.submit_batch([small]))
    assert u is None and z is None and same_features(k[0, :n[0]], d[0, :n[0]], ok0, od0)
    first_call_again("after the mono ticket")


def test_reconfiguration_resets_what_the_last_call_left(gpu):
    """Between a (re)configuration and the next call the handle reports the planned pyramid launches of the CURRENT geometry, not the count of the
    last call on the previous one; a refused geometry leaves a handle that extracts as a fresh one does."""
    s = HS.FeatureExtractorSettings(nFeatures=NF)
    img = synth_image(21, W1, H1)
    fresh = HS.ORBExtractor(s)
    fk, fd = fresh.extract_batch([img])
    assert len(fk[0]) > 200

    planned = HS.ORBExtractor(s)
    planned.reserve(W0, H0, 1)

    ex = HS.ORBExtractor(s)
    k, d = ex.extract_batch([img])
    assert same_features(k[0], d[0], fk[0], fd[0])
    ex.reserve(W0, H0, 1)
    assert ex.pyramid_launches() == planned.pyramid_launches()

    with pytest.raises(N.HsError) as e:
        ex.reserve(100, 400, 1)                      # aspect below 0.5: refused by the plan
    assert e.value.status == N.HS_ERR_INVALID
    k, d = ex.extract_batch([img])
    assert same_features(k[0], d[0], fk[0], fd[0])
