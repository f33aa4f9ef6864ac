"""GPU: the stages after the two track functions (include/hyslam_amd.h, "after the two track functions") against tests/ref_keyframe.py, which
tests/test_keyframe_ref.py pins on the CPU.

  * every directed case of tests/keyframe_cases.py through hs_track_keyframe_device and through the six stage entry points one by one, each from the
    state and the result the previous one left: every integer and flag equal, new_pos and the creation records bit-identical
  * 8 seeded cases, through the composite and stage by stage alike, at n = 1, 63, 64, 65, 1025, 2049 (the wave, the ranking kernel's 256-thread tile + 1, more than one trip of the 1024-thread
    passes), reference key frames of 0, 1 and 1025 keypoints, new_cap below, at and above n_new; the same call twice gives the same bytes
  * hs_track_frame_device -> hs_track_keyframe_device -> hs_landmark_update_entries_device scattering into d_lms[L .. L + n_new), against
    tests/ref_landmark_entry.py fed the same records
  * FrameTracker.KeyFrameDecision returns the same; bad arguments are refused before anything is enqueued
Every device output has guard bytes behind it, checked on every read."""
import numpy as np
import pytest

import hipmem
import keyframe_cases as KC
import ref_keyframe as RKF
from chain_compare import compare_keyframe as compare

pytestmark = pytest.mark.gpu

GUARD = 64
SIZES = KC.GPU_SIZES


@pytest.fixture(scope="module")
def tracker(gpu):
    import hyslam_amd as HS
    return HS.FrameTracker(HS.ORBExtractor(device=0))


def dev(a):
    a = np.ascontiguousarray(a)
    return hipmem.DevBuf.from_numpy(a) if a.nbytes else hipmem.DevBuf(64)


def out_buf(nbytes):
    b = hipmem.DevBuf(nbytes + GUARD)
    b.fill(0x55)
    return b


def put(buf, a):
    a = np.ascontiguousarray(a)
    if a.nbytes:
        hipmem._ok(hipmem.hip().hipMemcpy(buf.ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")


def guarded(a):
    a = np.ascontiguousarray(a)
    b = out_buf(a.nbytes)
    put(b, a)
    return b


def read(buf, dtype, count):
    nbytes = np.dtype(dtype).itemsize * count
    raw = buf.to_numpy(np.uint8, nbytes + GUARD)
    assert (raw[nbytes:] == 0x55).all(), "bytes written behind the output"
    return raw[:nbytes].view(dtype).copy()


class Dev:
    """one case on the device: inputs, the state, every output buffer (guarded) and the work area"""

    def __init__(self, tracker, c):
        from hyslam_amd import _native as N
        self.N, self.tr, self.c = N, tracker, c
        fr, T, K = c["frame"], c["T"], c["K"]
        self.n, self.L, self.new_cap = len(c["depth"]), len(T["lm_nobs"]), c["new_cap"]
        F = N.FrameView()
        F.fx, F.fy, F.cx, F.cy, F.mbf, F.sensor = fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["mbf"], fr["sensor"]
        F.min_x, F.max_x, F.min_y, F.max_y = fr["bounds"]
        F.size_ref, F.n = 31.0, self.n
        self.fkeep = [dev(np.ascontiguousarray(fr["kps"], N.KP_DTYPE)), dev(np.ascontiguousarray(fr["desc"], np.uint8))]
        F.kps, F.desc = (b.ptr for b in self.fkeep)
        self.F = F
        order = ("lm_obs_offsets", "lm_obs_kf", "lm_obs_octave", "lm_bad", "lm_nobs", "kf_bad", "kf_id")
        self.tkeep = [dev(T[k]) for k in order]
        self.KT = N.KfTable(self.L, len(T["kf_id"]), *[b.ptr for b in self.tkeep])
        self.kkeep = [dev(np.asarray(K["kf_off"], np.int64)), dev(np.asarray(K["kp_lm"], np.int32))]
        self.KF = N.KfFeatures(K["n_kf"], self.kkeep[0].ptr, None, None, None, self.kkeep[1].ptr, None)
        self.d_depth, self.d_T = dev(np.asarray(c["depth"], np.float32)), dev(np.asarray(c["Tcw"], np.float32))
        tr = np.zeros(1, N.TRACK_RESULT_DTYPE)
        for k in ("status", "n_matches_map", "n_inliers"):
            tr[k] = c["track"][k]
        self.d_track = dev(tr)
        p = c["prm"]
        self.prm = N.KeyFrameParams(**p)
        # kp_lm_obs starts dirty: stage 1 rewrites all of it
        self.state = [guarded(c["state"][0]), guarded(c["state"][1]), guarded(np.array([c["state"][2]], np.int32)), guarded(np.full(self.n, 7, np.int32))]
        self.ST = N.TrackState(*[b.ptr for b in self.state])
        self.d_ref = guarded(np.array([c["ref_slot"]], np.int32))
        self.out, self.obufs = tracker.keyframe_outputs(self.new_cap, alloc=out_buf)
        self.work_bytes = tracker.keyframe_work_bytes(self.n, self.KT.n_kf, self.new_cap)
        self.work = out_buf(self.work_bytes)
        self.stream = hipmem.Stream()

    @property
    def d_result(self):
        return self.obufs["result"][0].ptr

    def composite(self):
        self.tr.track_keyframe_device(self.F, self.d_depth.ptr, self.d_T.ptr, self.KT, self.KF, self.d_track.ptr, self.prm, self.ST, self.d_ref.ptr, self.new_cap,
                                      self.out, self.work.ptr, self.stream.ptr)

    def stage(self, s):
        tr, st = self.tr, self.stream.ptr
        if s == 1:
            tr.keyframe_reference_device(self.n, self.ST, self.KT, self.d_ref.ptr, self.d_result, self.work.ptr, st)
        elif s == 2:
            tr.keyframe_gate_device(self.d_track.ptr, self.prm, self.d_result, st)
        elif s == 3:
            tr.keyframe_clean_device(self.n, self.ST, self.KT, self.d_result, st)
        elif s == 4:
            tr.keyframe_need_device(self.n, self.F.sensor, self.d_depth.ptr, self.ST, self.KT, self.KF, self.d_ref.ptr, self.d_track.ptr, self.prm, self.d_result, st)
        elif s == 5:
            tr.keyframe_create_device(self.F, self.d_depth.ptr, self.d_T.ptr, self.ST, self.KT, self.prm, self.new_cap, self.out, self.work.ptr, st)
        else:
            tr.keyframe_discard_device(self.n, self.ST, self.d_result, st)

    def results(self):
        self.stream.synchronize()
        read(self.work, np.uint8, self.work_bytes)
        got = {k: read(b, dt, cnt) for k, (b, dt, cnt) in self.obufs.items()}
        got["kp_lm"], got["kp_outl"] = read(self.state[0], np.int32, self.n), read(self.state[1], np.uint8, self.n)
        got["n_matches"], got["kp_lm_obs"] = int(read(self.state[2], np.int32, 1)[0]), read(self.state[3], np.int32, self.n)
        got["ref_slot_mem"] = int(read(self.d_ref, np.int32, 1)[0])
        return got


def stagewise(tracker, c, want, tag, ref):
    """the six entry points one by one: each from what the previous one left on the device, against the reference stage (`ref`) fed the same"""
    d, cur, res = Dev(tracker, c), dict(c), {k: 0 for k in RKF.RESULT_KEYS}
    put(d.obufs["result"][0], np.zeros(1, d.N.KEYFRAME_RESULT_DTYPE))
    for s in range(1, 7):
        d.stage(s)
        w = ref(cur, stages=(s,), res=res)
        compare(d.results(), w, c["new_cap"], (tag, s), stages=(s,))
        cur = dict(cur, state=(w["kp_lm"], w["kp_outl"], w["n_matches"]), ref_slot=w["result"]["ref_slot"], kp_lm_obs=w["kp_lm_obs"])
        res = w["result"]
    assert res == want["result"], tag
    for k in ("kp_lm", "kp_outl", "n_matches", "kp_lm_obs"):
        assert np.array_equal(w[k], want[k]), (tag, k)


@pytest.mark.parametrize("name", sorted(KC.DIRECTED))
def test_directed(tracker, name):
    c, witness = KC.DIRECTED[name]
    want = RKF.literal(c)
    assert witness(want)
    d = Dev(tracker, c)
    d.composite()
    compare(d.results(), want, c["new_cap"], name)
    stagewise(tracker, c, want, name, RKF.literal)


@pytest.mark.parametrize("n", SIZES)
def test_seeded(tracker, n):
    first = None
    for seed in range(8):
        c = KC.gpu_seeded(n, seed)
        want = RKF.dense(c)                      # test_keyframe_ref.py holds it equal to the sequential walk on exactly these cases, at every size
        d = Dev(tracker, c)
        d.composite()
        got = d.results()
        compare(got, want, c["new_cap"], (n, seed))
        stagewise(tracker, c, want, (n, seed), RKF.dense)
        if seed == 0:
            first = (c, got)
    c, got = first                                                              # the same call again: the same bytes
    d = Dev(tracker, c)
    d.composite()
    again = d.results()
    for k in got:
        assert np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes(), (n, k)


def test_chain_track_then_keyframe_then_entry_update(tracker):
    """hs_track_frame_device -> hs_track_keyframe_device -> hs_landmark_update_entries_device on one stream, no host step in between: the new records
    d_lms[L .. L + n_new) hold pos (stage 5) and normal, distances, size, descriptor (the entry update), as ref_landmark_entry computes from the records"""
    import ref_landmark_entry as RL
    import track_cases as TC
    from test_gpu_track import Chain
    from hyslam_amd import _native as N
    c = TC.build(91, n=130, n_last=90, extra=40)
    ch = Chain(tracker, c)
    fr, n, L = c["frame"], ch.n, ch.L
    with np.errstate(all="ignore"):
        depth = np.where(fr["uR"] > 0, np.float32(fr["mbf"]) / (fr["kps"]["x"] - fr["uR"]).astype(np.float32), np.float32(-1)).astype(np.float32)
    rng = np.random.default_rng(4)
    K = KC.keyframes([rng.integers(-1, L, 70).tolist() for _ in range(len(c["T"]["kf_id"]))])
    prm = RKF.params(force=1, th_depth=float(np.nanmedian(depth[depth > 0])), n_min_points=20, thresh_init=5, thresh_refine=5)
    new_cap = n
    kkeep = [dev(K["kf_off"]), dev(K["kp_lm"])]
    KF = N.KfFeatures(K["n_kf"], kkeep[0].ptr, None, None, None, kkeep[1].ptr, None)
    d_depth, d_ref = dev(depth), guarded(np.array([-1], np.int32))
    out, obufs = tracker.keyframe_outputs(new_cap, alloc=out_buf)
    for k in ("entries", "obs", "desc"):                                        # records behind n_new are read by the entry update (and scattered nowhere)
        obufs[k][0].fill(0)
    lms_big = np.zeros(L + new_cap, N.LM_DTYPE)
    lms_big[:L] = c["lms"]
    lms_big["skip"][L:] = 1
    d_lms_big = guarded(lms_big)
    out.lms, out.lms_cap = d_lms_big.ptr, L + new_cap
    work = out_buf(tracker.keyframe_work_bytes(n, ch.KT.n_kf, new_cap))
    eouts = [out_buf(new_cap * 12)] + [out_buf(new_cap * 4) for _ in range(7)]
    s = ch.stream.ptr
    ch.frame()
    d_Tcw = ch.ptr("pose_local") + N.POSE_RESULT_DTYPE.fields["Tcw"][1]
    tracker.track_keyframe_device(ch.F, d_depth.ptr, d_Tcw, ch.KT, KF, ch.ptr("result"), N.KeyFrameParams(**prm), ch.ST, d_ref.ptr, new_cap, out, work.ptr, s)
    tracker._ex.landmark_update_entries_device(new_cap, obufs["entries"][0].ptr, obufs["obs_offsets"][0].ptr, obufs["obs"][0].ptr, obufs["desc_offsets"][0].ptr,
                                               obufs["desc"][0].ptr, *[o.ptr for o in eouts], d_lms=d_lms_big.ptr, d_lm_index=obufs["lm_index"][0].ptr,
                                               n_lms=L + new_cap, stream=s)
    ch.stream.synchronize()
    # the reference, from what the tracking chain left on the device: its state is the keyframe stage's input
    tres = read(ch.spec["result"][0], N.TRACK_RESULT_DTYPE, 1)[0]
    pose = read(ch.spec["pose_local"][0], N.POSE_RESULT_DTYPE, 1)[0]
    lm_index = read(obufs["lm_index"][0], np.int32, new_cap)
    res = read(obufs["result"][0], N.KEYFRAME_RESULT_DTYPE, 1)[0]
    final = (read(ch.state[0], np.int32, n), read(ch.state[1], np.uint8, n), int(read(ch.state[2], np.int32, 1)[0]))
    # the tracking chain once more, on its own: the state BEFORE the keyframe stages (the chain gives the same bytes every time)
    ch2 = Chain(tracker, c)
    ch2.frame()
    g2 = ch2.results()
    case = dict(state=(g2["kp_lm"], g2["kp_outl"], int(g2["n_matches"][0])), T=c["T"], K=K, depth=depth, frame=fr, Tcw=pose["Tcw"].reshape(4, 4),
                track=dict(status=int(tres["status"]), n_matches_map=int(tres["n_matches_map"]), n_inliers=int(tres["n_inliers"])), prm=prm, ref_slot=-1,
                new_cap=new_cap)
    want = RKF.literal(case)
    assert want["result"]["ok"] == 1 and want["result"]["insert"] == 1 and 5 < want["result"]["n_new"] < new_cap
    assert want["result"]["n_processed"] < want["result"]["n_candidates"], "the walk is cut in this case"
    assert {k: int(res[k]) for k in RKF.RESULT_KEYS} == want["result"]
    for g, w in zip(final, (want["kp_lm"], want["kp_outl"], want["n_matches"])):
        assert np.array_equal(g, w)
    assert np.array_equal(lm_index, want["lm_index"])
    m = want["result"]["n_new"]
    ref = RL.update_entries(want["entries"], [want["obs"][k:k + 1] for k in range(m)], [want["desc"][k:k + 1] for k in range(m)])
    got = read(d_lms_big, N.LM_DTYPE, L + new_cap)
    assert got[:L].tobytes() == lms_big[:L].tobytes() and got[L + m:].tobytes() == lms_big[L + m:].tobytes()
    exp = lms_big[L:L + m].copy()
    exp["pos"], exp["assoc_kp"], exp["prev_angle"], exp["skip"] = want["new_pos"], -1, 0, 0
    exp["normal"], exp["min_dist"], exp["max_dist"], exp["size"], exp["desc"] = ref["normal"], ref["min_dist"], ref["max_dist"], ref["size"], want["desc"]
    assert (ref["flags"] & RL.HS_LM_SET_NORMAL_DEPTH).all() and (ref["best"] == 0).all()
    for f in exp.dtype.names:
        assert RL.same(got[L:L + m][f], exp[f]), f


def test_python_method(tracker):
    c = KC.seeded(7801, 65, force=1)
    want = RKF.literal(c)
    from hyslam_amd import _native as N
    r = tracker.KeyFrameDecision(c["frame"], c["depth"], c["Tcw"], c["T"], c["K"], *c["state"], c["ref_slot"], track_result=c["track"],
                                 params=N.KeyFrameParams(**c["prm"]), new_cap=c["new_cap"])
    assert {k: r[k] for k in RKF.RESULT_KEYS} == want["result"] and want["result"]["n_new"] > 3
    for k in ("kp_lm", "kp_outl", "kp_lm_obs", "new_view", "lm_index", "offsets"):
        assert np.array_equal(r[k], want[k]), k
    assert r["n_matches"] == want["n_matches"]
    for k in ("new_pos", "entries", "obs", "desc"):
        assert np.asarray(r[k]).tobytes() == np.asarray(want[k]).tobytes(), k


def test_refusals(tracker):
    from hyslam_amd import _native as N
    import hyslam_amd as HS
    c = KC.DIRECTED["equal_depths"][0]
    d = Dev(tracker, c)
    bad_state = N.TrackState(d.state[0].ptr, None, d.state[2].ptr, d.state[3].ptr)
    no_override = N.KeyFrameParams(**c["prm"])
    no_offsets = N.KfTable.from_buffer_copy(d.KT)                               # what only the vote reads is checked before stage 1's first launch too
    no_offsets.lm_obs_offsets = None
    no_kf_bad = N.KfTable.from_buffer_copy(d.KT)
    no_kf_bad.kf_bad = None
    calls = [lambda: d.tr.keyframe_reference_device(0, d.ST, d.KT, d.d_ref.ptr, d.d_result, d.work.ptr),
             lambda: d.tr.keyframe_reference_device(65536, d.ST, d.KT, d.d_ref.ptr, d.d_result, d.work.ptr),
             lambda: d.tr.keyframe_clean_device(d.n, bad_state, d.KT, d.d_result),
             lambda: d.tr.keyframe_reference_device(d.n, d.ST, no_offsets, d.d_ref.ptr, d.d_result, d.work.ptr),
             lambda: d.tr.track_keyframe_device(d.F, d.d_depth.ptr, d.d_T.ptr, no_kf_bad, d.KF, d.d_track.ptr, d.prm, d.ST, d.d_ref.ptr, d.new_cap, d.out, d.work.ptr),
             lambda: d.tr.keyframe_gate_device(None, no_override, d.d_result),
             lambda: d.tr.track_keyframe_device(d.F, None, d.d_T.ptr, d.KT, d.KF, d.d_track.ptr, d.prm, d.ST, d.d_ref.ptr, d.new_cap, d.out, d.work.ptr),
             lambda: d.tr.track_keyframe_device(d.F, d.d_depth.ptr, d.d_T.ptr, d.KT, d.KF, d.d_track.ptr, d.prm, d.ST, d.d_ref.ptr, -1, d.out, d.work.ptr)]
    for i, call in enumerate(calls):
        with pytest.raises(HS.HsError):
            call()
    got = d.results()                                                           # nothing was enqueued: the state and the outputs are untouched
    assert np.array_equal(got["kp_lm"], c["state"][0]) and (got["result"].view(np.uint8) == 0x55).all()
