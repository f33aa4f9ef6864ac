"""k_stereo_match_compact<4> / <8> (HS_STEREO_KPW=4 / 8: the gated candidates of K left keypoints queue up in LDS, the distances are formed on
dense lanes) through hs_stereo_match_batch_device: every result bit-identical to the CPU oracle, and the full [pairs][cap] arrays, written into
buffers pre-filled with a sentinel, byte-identical to the HS_STEREO_KPW=2 run (k_stereo_match<2>).  Wave boundaries, a strip that overflows the
queue several times per wave, equal distances across queue drains, TH_LOW > TH_HIGH, invalid keypoints beside valid ones in one wave, and the
by-batch choice of the instance with the knob unset."""
import numpy as np
import pytest

import hipmem
import oracle
import scenes
import hyslam_amd as HS
from hyslam_amd import _native as N

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-777.25)
BY_BATCH_STEPS = (6 * 2048, 24 * 2048)      # pairs * cap from which the by-batch choice runs k_stereo_match_compact<4> and <8> (kernels_stereo.hip: hs_stereo_kpw)
BASE = dict(fx=500.0, mbf=60.0, n_rows=480, th_high=100.0, th_low=50.0, size_ref=31.0)


@pytest.fixture(scope="module")
def handle():
    """handle(kpw): an extractor handle created with HS_STEREO_KPW = kpw (None: unset) — the knob is read when the handle is created"""
    made = {}

    def get(kpw):
        if kpw not in made:
            with pytest.MonkeyPatch.context() as mp:
                if kpw is None:
                    mp.delenv("HS_STEREO_KPW", raising=False)
                else:
                    mp.setenv("HS_STEREO_KPW", str(kpw))
                made[kpw] = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=1000))
        return made[kpw]
    return get


def device_run(ex, cases, cap, params):
    """hs_stereo_match_batch_device on `cases` [(kL, dL, kR, dR)] laid out with stride cap; the full (uRight, depth) arrays [pairs][cap]"""
    P = len(cases)
    kL, kR = np.zeros((P, cap), N.KP_DTYPE), np.zeros((P, cap), N.KP_DTYPE)
    dL, dR = np.zeros((P, cap, 32), np.uint8), np.zeros((P, cap, 32), np.uint8)
    nL, nR = np.zeros(P, np.int32), np.zeros(P, np.int32)
    for j, (a, b, c, d) in enumerate(cases):
        nL[j], nR[j] = len(a), len(c)
        kL[j, :len(a)], dL[j, :len(a)], kR[j, :len(c)], dR[j, :len(c)] = a, b, c, d
    bufs = [hipmem.DevBuf.from_numpy(x) for x in (kL, dL, nL, kR, dR, nR)]
    d_u, d_z = (hipmem.DevBuf.from_numpy(np.full(P * cap, SENTINEL, np.float32)) for _ in range(2))
    sp = N.StereoParams(params["fx"], params["mbf"], params["n_rows"], params["th_high"], params["th_low"], params["size_ref"])
    ex.stereo_match_batch_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, P, cap, sp, d_u.ptr, d_z.ptr, 0)
    ex.synchronize()
    return d_u.to_numpy(np.float32, P * cap).reshape(P, cap), d_z.to_numpy(np.float32, P * cap).reshape(P, cap)


def check(handle, kpw, cases, cap, params, what, refs=None):
    """the run of the handle with HS_STEREO_KPW = kpw: every pair against the oracle (`refs`: its results where the caller already has them), slots
    at and beyond nL at -1, the whole arrays against the HS_STEREO_KPW=2 run.  Returns (uRight, depth) of the run and the oracle's results per pair."""
    u, z = device_run(handle(kpw), cases, cap, params)
    u2, z2 = device_run(handle(2), cases, cap, params)
    if refs is None:
        refs = [oracle.stereo_match(a, b, c, d, oracle.stereo_params(**params)) for a, b, c, d in cases]
    for j, (a, b, c, d) in enumerate(cases):
        ou, oz, obi, obd = refs[j]
        n = len(a)
        bad = np.nonzero((u[j, :n].view(np.uint32) != ou.view(np.uint32)) | (z[j, :n].view(np.uint32) != oz.view(np.uint32)))[0]
        assert len(bad) == 0, "%s, KPW %s, pair %d of %d (nL %d, nR %d), cap %d: %d keypoints differ; first iL=%d: device (uR %r, depth %r), oracle (uR %r, depth %r, best iR %d at distance %d)" % (
            what, kpw, j, len(cases), n, len(c), cap, len(bad), bad[0], u[j, bad[0]], z[j, bad[0]], ou[bad[0]], oz[bad[0]], obi[bad[0]], obd[bad[0]])
        assert (u[j, n:] == -1).all() and (z[j, n:] == -1).all(), "%s, KPW %s, pair %d: slots at and beyond nL" % (what, kpw, j)
    assert u.tobytes() == u2.tobytes() and z.tobytes() == z2.tobytes(), "%s: KPW %s against KPW 2" % (what, kpw)
    return u, z, refs


def edge_cases(rng, sizes, params, kinds=scenes.STEREO_EDGE_KINDS):
    out = []
    for j, (nl, nr) in enumerate(sizes):
        kL, dL, kR, dR, _ = scenes.stereo_edge_lists(rng, kinds[j % len(kinds)], nL=nl, nR=nr, n_rows=params["n_rows"], size_ref=params["size_ref"],
                                                     th=(params["th_high"], params["th_low"]), fx=params["fx"])
        out.append((kL, dL, kR, dR))
    return out


def dense_lists(rng, nL=600, nR=600, bases=0, dist=0):
    """Every right keypoint is a candidate of every left keypoint: all rows in strip 1 (rows 41 .. 43 inside every band [40, 44] at size 31 =
    size_ref), one octave, uR in [100, 300) left of uL in [300, 590] with maxD = fx = 500.  Distinct uR, so that uRight names the winner.
    bases > 0: the descriptors are drawn from `bases` patterns, left ones with `dist` bits flipped — many right keypoints at one distance."""
    kL, kR = np.zeros(nL, oracle.KP_DTYPE), np.zeros(nR, oracle.KP_DTYPE)
    for k, n, x in ((kL, nL, rng.uniform(300, 590, nL)), (kR, nR, rng.permutation(nR) / 3.0 + 100.0)):
        k["x"], k["size"], k["octave"], k["response"] = x, 31.0, 0, 50.0
        k["angle"] = rng.uniform(0, 360, n)
    kL["y"] = rng.choice([41.0, 42.25, 43.5], nL)
    kR["y"] = 42.0
    if bases:
        pat = rng.integers(0, 256, (bases, 32), dtype=np.uint8)
        dR = pat[rng.integers(0, bases, nR)]
        dL = scenes.flip_bits(rng, pat[rng.integers(0, bases, nL)], dist)
    else:
        dL = rng.integers(0, 256, (nL, 32), dtype=np.uint8)
        dR = rng.integers(0, 256, (nR, 32), dtype=np.uint8)
        own = rng.random(nR) < 0.5                           # half of the right descriptors are a left one with a few bits flipped
        dR[own] = scenes.flip_bits(rng, dL[rng.integers(0, nL, int(own.sum()))], rng.integers(0, 60, int(own.sum())))
    return kL, dL, kR, dR


@pytest.mark.parametrize("K", [4, 8])
def test_wave_boundaries(gpu, handle, K):
    """nL around one wave's K keypoints, nR of 0, 1 and many, caps that are no multiple of K, an empty pair between full ones"""
    rng = np.random.default_rng(4100 + K)
    for cap, many in ((1001, 700), (301, 301)):
        sizes = [(cap, cap), (0, 0), (cap, many)] + [(nl, nr) for nl in (0, 1, K - 1, K, K + 1) for nr in (0, 1, many)] + [(cap - 1, 1), (4 * K + 1, cap)]
        params = dict(BASE, size_ref=7.5, th_low=51.0)
        check(handle, K, edge_cases(rng, sizes, params), cap, params, "wave boundaries")


@pytest.mark.parametrize("K", [4, 8])
def test_queue_drain(gpu, handle, K):
    """600 x 600, every candidate passes the gate: five gate rounds per keypoint (nc > 128), 600 K entries through a queue of 192; with
    TH_HIGH = 257 every one of them also reaches the minimum"""
    rng = np.random.default_rng(4200 + K)
    case = dense_lists(rng)
    for th in ((100.0, 50.0), (257.0, 256.0)):
        params = dict(BASE, th_high=th[0], th_low=th[1])
        _, _, ((ou, oz, obi, obd),) = check(handle, K, [case], 600, params, "queue drain %r" % (th,))
        assert (oz > 0).sum() > 100                                # the case has matches to lose


@pytest.mark.parametrize("K", [4, 8])
def test_ties_smallest_index_wins(gpu, handle, K):
    """~85 right keypoints at the minimum distance of every left keypoint, at indices all over the list and so in different queue drains: the
    smallest iR wins (the uR values are distinct: uRight names the winner).  Then the generated `ties` lists."""
    rng = np.random.default_rng(4300 + K)
    bits = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1)
    for dist in (3, 7):
        kL, dL, kR, dR = case = dense_lists(rng, bases=7, dist=dist)
        params = dict(BASE, th_high=257.0, th_low=256.0)            # everything accepted; every best distance = dist < 2.1 * dist, the median cut
        u, _, _ = check(handle, K, [case], 600, params, "ties at distance %d" % dist)
        d = bits[dL[:, None, :] ^ dR[None, :, :]].sum(2)
        assert (d.min(1) == dist).all() and ((d == dist).sum(1) > 40).all()
        assert np.array_equal(u[0], kR["x"][d.argmin(1)]), "distance %d" % dist       # numpy's argmin: the first minimum
    params = dict(BASE, size_ref=4.0)
    check(handle, K, edge_cases(rng, [(333, 500)] * 4, params, kinds=("ties",)), 501, params, "generated ties")


@pytest.mark.parametrize("K", [4, 8])
def test_th_low_above_th_high(gpu, handle, K):
    """th = (80, 120), accepted below 100: a keypoint with candidates in its band but none under TH_HIGH keeps the reference's initial bestDist =
    TH_HIGH, bestIdxR = 0 and is paired with right keypoint 0; one without any candidate is not; a real match stays — all three kinds in every
    wave.  (The median of the accepted distances is TH_HIGH here, so its cut keeps them all.)"""
    rng = np.random.default_rng(4400 + K)
    params = dict(BASE, th_high=80.0, th_low=120.0)
    nL = 3 * K + 1
    idx = np.arange(nL)
    kind = idx % 3                                                  # 0: in-band candidates, none under TH_HIGH; 1: no candidate; 2: a real match
    kL, kR = np.zeros(nL, oracle.KP_DTYPE), np.zeros(2 * nL + 1, oracle.KP_DTYPE)
    kL["x"], kL["size"] = 400.0 + idx, 31.0
    kL["y"] = np.where(kind == 1, 300.5, 42.0 + 64.0 * (idx % 2))   # rows 42 and 106 (strips 1 and 3); row 300 has no right keypoint near it
    dL = rng.integers(0, 256, (nL, 32), dtype=np.uint8)
    kR["size"] = 31.0
    kR["x"][0], kR["y"][0] = 350.0, 42.0                            # right keypoint 0: a disparity of 50 + iL
    a, b = kR[1::2], kR[2::2]                                       # (views) two right keypoints per left one:
    a["x"], a["y"], a["octave"] = 390.0, np.where(kind == 1, 42.0, kL["y"]), 5          # in the left row's band, outside its octave window
    b["x"], b["y"] = 380.0 + idx / 4.0, np.where(kind == 2, kL["y"], 42.0)              # kind 2: the match, 5 bits away; else the complement
    dR = rng.integers(0, 256, (2 * nL + 1, 32), dtype=np.uint8)
    dR[2::2] = np.where((kind == 2)[:, None], scenes.flip_bits(rng, dL, 5), 255 - dL)
    case = (kL, dL, kR, dR)
    u, z, ((ou, oz, obi, obd),) = check(handle, K, [case], 2 * nL + 1, params, "TH_LOW > TH_HIGH")
    assert (u[0, :nL][kind == 1] == -1).all()
    assert np.array_equal(u[0, :nL][kind == 2], b["x"][kind == 2]) and (u[0, :nL][kind == 0] == np.float32(350.0)).all()
    params = dict(BASE, th_high=80.0, th_low=120.0, size_ref=7.5)
    check(handle, K, edge_cases(rng, [(2 * K + 1, 300), (150, 301)], params), 301, params, "generated lists at th (80, 120)")


@pytest.mark.parametrize("n_rows", [0, 33, 480])
@pytest.mark.parametrize("K", [4, 8])
def test_mixed_validity_in_one_wave(gpu, handle, K, n_rows):
    """rows below 0 and at or above n_rows, maxU < 0 and keypoints of different strips side by side in every wave"""
    rng = np.random.default_rng(4500 + 10 * K + n_rows)
    params = dict(BASE, n_rows=n_rows, size_ref=7.5)
    cases = edge_cases(rng, [(5 * K + 3, 400), (2 * K, 77)], params, kinds=("clip", "mixed"))
    rows = np.array([-2.5, n_rows + 0.5, 3.0, float(n_rows), 17.25, n_rows - 0.5, 31.75, 32.0, -0.25, 100.0], np.float32)
    for kL, dL, kR, dR in cases:
        kL["y"] = rows[np.arange(len(kL)) % len(rows)]
        kL["x"][2::7] = -1.5                                         # maxU < 0
        kR["y"][::3] = rng.choice([2.0, 17.0, 31.0, 32.5, n_rows - 1.0], len(kR[::3]))
    _, _, refs = check(handle, K, cases, 403, params, "mixed validity, n_rows %d" % n_rows)
    if n_rows == 0:
        assert all((r[1] == -1).all() for r in refs)
    else:
        assert (refs[0][1] > 0).any()                                # valid keypoints with a match stand beside the invalid ones


def test_by_batch_choice_crosses_the_thresholds(gpu, handle):
    """the knob unset: pairs * cap one pair below and at each step of the by-batch choice (k_stereo_match<1> -> k_stereo_match_compact<4> -> <8>), every run against
    the oracle and against the HS_STEREO_KPW=2 handle"""
    rng = np.random.default_rng(4600)
    cap = 2048
    params = dict(BASE, n_rows=1080, fx=1050.0, mbf=126.0)
    pool = edge_cases(rng, [(2048, 2048), (700, 1500), (0, 0), (1, 2048), (2047, 3), (1023, 1999)], params)
    pool_refs = [oracle.stereo_match(a, b, c, d, oracle.stereo_params(**params)) for a, b, c, d in pool]
    for step in BY_BATCH_STEPS:
        assert step % cap == 0
        for pairs in (step // cap - 1, step // cap):
            pick = [j % len(pool) for j in range(pairs)]
            check(handle, None, [pool[j] for j in pick], cap, params, "%d pairs by batch" % pairs, refs=[pool_refs[j] for j in pick])
