"""GPU: every entry point that carves a caller-owned work area (hyslam_amd/csrc/hs_work.h), at the smallest shapes at which a wrong carve shows: the two
replays at n = 1 and around one wave, the key-frame stages where 8 n crosses a multiple of 256, L around 256 everywhere and around one block of
HS_LOCAL_POINTS_BLOCK for the local points.  d_work is devbuf.out_buf at exactly the public size (pattern-filled, guard bytes behind it, checked on
read); results against the Python references on cases from the existing builders.  An overlap of two sub-arrays or a carve past the size shows as a
wrong result or a touched guard.  tests/test_work_bytes.py checks the same layouts on the CPU."""
import numpy as np
import pytest

import hipmem
import keyframe_cases as KC
import ref_keyframe as RKF
import ref_kfgraph as RK
import ref_localmap as RL
import ref_refkf as RR
import ref_track as R
import refkf_cases as RC
import track_cases as TC
from chain_compare import compare_keyframe
from devbuf import dev, guarded, out_buf, read
from kfgraph_cases import random_table
from localmap_cases import random_points

pytestmark = pytest.mark.gpu

REPLAY_N = [1, 63, 64, 65]
AROUND_256 = [1, 255, 256, 257]
AROUND_A_BLOCK = [1023, 1024, 1025]


@pytest.fixture(scope="module")
def tracker(gpu):
    import hyslam_amd as HS
    return HS.FrameTracker(HS.ORBExtractor(device=0))


def _state(s):
    return guarded(s["kp_lm"]), guarded(s["kp_outl"]), guarded(np.array([s["n_matches"]], np.int32))


def _dense(bufs, n):
    return read(bufs[0], np.int32, n), read(bufs[1], np.uint8, n), int(read(bufs[2], np.int32, 1)[0])


def _with_an_op(s):
    """the builders draw no op where n or L is 1: such a state gets one, view 0 takes landmark 0"""
    if not ((s["op_view"] >= 0) & (s["op_lm"] >= 0)).any():
        s["op_view"][0], s["op_lm"][0] = 0, 0
    return s


def _same_state(got, want, tag):
    for g, w, what in zip(got, want, ("kp_lm", "kp_outl", "n_matches")):
        assert np.array_equal(g, w), (what,) + tag


@pytest.mark.parametrize("L", AROUND_256)
@pytest.mark.parametrize("n", REPLAY_N)
def test_replay_in_landmark_order(tracker, n, L):
    s = _with_an_op(TC.replay_state(41000 + 1000 * n + L, n, n, L))
    want = R.replay_sequential(R.MapMatches.from_dense(s["kp_lm"], s["kp_outl"], s["n_matches"]), s["op_view"], s["op_lm"], n, L).dense(n)
    st, ops, nbytes = _state(s), (dev(s["op_view"]), dev(s["op_lm"])), tracker.track_work_bytes(n, 0, L, 0)
    work, stream = out_buf(nbytes), hipmem.Stream()
    tracker.frame_associate_device(n, L, st[0].ptr, st[1].ptr, st[2].ptr, n, ops[0].ptr, ops[1].ptr, work.ptr, stream.ptr)
    stream.synchronize()
    read(work, np.uint8, nbytes)
    _same_state(_dense(st, n), want, (n, L))


@pytest.mark.parametrize("L", AROUND_256)
@pytest.mark.parametrize("n", REPLAY_N)
def test_replay_in_view_order(tracker, n, L):
    s = _with_an_op(RC.replay_state(42000 + 1000 * n + L, n, L))
    want = RR.replay_views_sequential(R.MapMatches.from_dense(s["kp_lm"], s["kp_outl"], s["n_matches"]), s["op_view"], s["op_lm"], n, L).dense(n)
    st, ops, nbytes = _state(s), (dev(s["op_view"]), dev(s["op_lm"])), tracker.track_refkf_work_bytes(n, 0, L)
    work, stream = out_buf(nbytes), hipmem.Stream()
    tracker.frame_associate_views_device(n, L, st[0].ptr, st[1].ptr, st[2].ptr, ops[0].ptr, ops[1].ptr, work.ptr, stream.ptr)
    stream.synchronize()
    read(work, np.uint8, nbytes)
    _same_state(_dense(st, n), want, (n, L))


def _table(T):
    """a table whose every landmark may be without observations: an empty array still needs an address"""
    from hyslam_amd import _native as N
    keep = [dev(T[k]) if len(T[k]) else hipmem.DevBuf(64) for k in ("lm_obs_offsets", "lm_obs_kf", "lm_obs_octave", "lm_bad", "lm_nobs", "kf_bad", "kf_id")]
    return N.KfTable(len(T["lm_bad"]), len(T["kf_id"]), *[b.ptr for b in keep]), keep


@pytest.mark.parametrize("L", AROUND_256 + AROUND_A_BLOCK)
def test_local_points(tracker, L):
    ex = tracker._ex
    T, local, flm = random_points(43007 + L, 12, L, max_obs=6, n_assoc=50)
    want = RL.local_points_fast(T, local, flm, L)
    assert L == 1 or (want["n_sel"] > 0 and want["frame_remove"].any()), "the case selects and removes"       # L = 1: the frame holds the one landmark
    KT, keep = _table(T)
    ins, nbytes = (dev(local), dev(flm)), ex.local_points_work_bytes(L)
    d_rem, d_sel, d_n, work, stream = out_buf(len(flm)), out_buf(L * 4), out_buf(4), out_buf(nbytes), hipmem.Stream()
    ex.local_points_device(KT, ins[0].ptr, ins[1].ptr, len(flm), d_rem.ptr, d_sel.ptr, L, d_n.ptr, work.ptr, stream.ptr)
    stream.synchronize()
    read(work, np.uint8, nbytes)
    got = dict(frame_remove=read(d_rem, np.uint8, len(flm)), sel=read(d_sel, np.int32, L), n_sel=int(read(d_n, np.int32, 1)[0]))
    assert RL.same(got, want) is None, L


@pytest.fixture(scope="module")
def search_scene():
    """one small stereo frame with landmarks around it, built once: every local-map case takes its first L landmarks"""
    import scenes
    from hyslam_amd import _native as N
    sc = scenes.projection_scene(71, 640, 480, nfeat=100, copies=3)
    lms = np.ascontiguousarray(sc["lms"], N.LM_DTYPE)
    assert len(lms) >= max(AROUND_256)
    return sc, lms


PROJ = (5.0, 100.0, 0.8, 0.5, 1.5, 1, 1, 0)                     # SearchByProjection(Frame, MapPoints, th = 5)


def local_map_case(scene, L, n_kf=20):
    """the first L landmarks of the scene under a random map of n_kf key frames, a frame that holds up to 40 of them, and the reference's answer to
    every stage of hs_local_map_search_device (cap = L)"""
    import oracle
    from test_oracle_matchers import py_search_by_projection
    sc, lms = scene
    lms, rng = lms[:L], np.random.default_rng(44000 + L)
    T = random_table(44000 + L, n_kf, L, max_obs=6, big=[(0, 3)], p_bad_lm=0.08, p_bad_kf=0.1)
    T["lm_bad"][0] = 0
    flm = rng.choice(L, min(L, 40), replace=False).astype(np.int32)
    flm[3::9] = -1
    neigh = rng.integers(-1, n_kf, (n_kf, 10)).astype(np.int32)
    parent = np.where(rng.random(n_kf) < 0.1, rng.integers(0, n_kf, n_kf), -1).astype(np.int32)
    held = flm[flm >= 0]
    w = RK.votes_fast(T, np.array([0, len(held)], np.int64), held, None, 1, 1, 0)
    want = dict(weights=w["weights"][0], max_slot=w["max_slot"][0], max_count=w["max_count"][0])
    want["local"], want["n_local"] = RL.local_keyframes_fast(want["weights"], T["kf_bad"], neigh, parent, 80, 10)
    pts = RL.local_points_fast(T, want["local"], flm, L)
    gathered = RL.gather(lms, pts["sel"], pts["n_sel"], L)
    matches = py_search_by_projection(sc["frame_args"], gathered, oracle.ProjParams(*PROJ))
    return dict(lms=lms, T=T, flm=flm, neigh=neigh, parent=parent, want=want, pts=pts, gathered=gathered, matches=matches)


@pytest.mark.parametrize("L", AROUND_256)
def test_local_map_search(tracker, search_scene, L):
    from hyslam_amd import _native as N
    from test_gpu_localmap import _device_frame, _outputs
    ex, n_kf, cap = tracker._ex, 20, L
    c = local_map_case(search_scene, L, n_kf)
    want, pts, flm = c["want"], c["pts"], c["flm"]
    assert want["n_local"] > 0 and (L == 1 or (pts["n_sel"] > 20 and len(c["matches"]) > 5)), "the case exercises every stage"
    KT, keep = _table(c["T"])
    Fd, fkeep = _device_frame(search_scene[0]["frame_args"])
    ins = dev(flm), dev(c["neigh"]), dev(c["parent"]), dev(c["lms"])
    spec, bufs, out = _outputs(dict(n_kf=n_kf, n_assoc=len(flm), cap=cap))
    nbytes = ex.local_map_work_bytes(L)
    work, stream = out_buf(nbytes), hipmem.Stream()
    ex.local_map_search_device(KT, ins[0].ptr, len(flm), ins[1].ptr, 10, ins[2].ptr, 80, 10, Fd, ins[3].ptr, N.ProjParams(*PROJ), cap, out, work.ptr, stream.ptr)
    stream.synchronize()
    read(work, np.uint8, nbytes)
    got = {k: read(bufs[k], dt, cnt) for k, dt, cnt in spec}
    for k in ("weights", "max_slot", "max_count", "local", "n_local"):
        assert np.array_equal(got[k].reshape(np.shape(want[k])), want[k]), (L, k)
    assert RL.same(dict(frame_remove=got["frame_remove"], sel=got["sel"], n_sel=int(got["n_sel"][0])), pts) is None, L
    assert got["lms"].tobytes() == c["gathered"].tobytes(), L
    found = {int(j): (int(got["match_idx"][j]), float(got["match_dist"][j])) for j in np.nonzero(got["match_idx"] >= 0)[0]}
    assert found == c["matches"] and int(got["n_matches"][0]) == len(c["matches"]), L


@pytest.mark.parametrize("L", AROUND_256)
@pytest.mark.parametrize("n", [31, 32, 33])
def test_keyframe_stages(tracker, n, L):
    """hs_keyframe_reference_device and hs_keyframe_create_device (stages 1 and 5) with the four stages around them, each from what the one before
    left on the device, against the reference stage fed the same"""
    from test_gpu_keyframe import Dev, put
    inserted = 0
    for seed in range(2):
        c = KC.seeded(45000 + 1000 * seed + 10 * n + L, n, L=L, n_kf=3)
        d = Dev(tracker, c)
        d.work = out_buf(d.work_bytes)
        assert d.work_bytes == tracker.keyframe_work_bytes(n, 3, c["new_cap"])
        put(d.obufs["result"][0], np.zeros(1, d.N.KEYFRAME_RESULT_DTYPE))
        cur, res = dict(c), {k: 0 for k in RKF.RESULT_KEYS}
        for s in range(1, 7):
            d.stage(s)
            w = RKF.dense(cur, stages=(s,), res=res)
            compare_keyframe(d.results(), w, c["new_cap"], (n, L, seed, s), stages=(s,))
            cur = dict(cur, state=(w["kp_lm"], w["kp_outl"], w["n_matches"]), ref_slot=w["result"]["ref_slot"], kp_lm_obs=w["kp_lm_obs"])
            res = w["result"]
        inserted += res["n_new"] > 0
    assert inserted, "no case of this shape created a landmark"
