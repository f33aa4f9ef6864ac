"""GPU: initial pose estimation as one resident call (hs_track_reference_keyframe_device, hs_track_initial_device, hs_track_normal_device;
include/hyslam_amd.h, DESIGN.md 5.13 "the chain") against tests/ref_refkf.py, which tests/test_refkf_ref.py pins on the CPU.  Every case comes from
tests/refkf_cases.py: 96 keypoints, 64 in the last frame, 160 landmarks, a store of three key frames (40 / 80 / 0 keypoints), kf_cap 80 and 50.

  1 against the reference   every directed and random case through hs_track_normal_device on a stream of its own: integers, bow_weight's bytes, the
                            state after both stages and the 32 result bytes exactly, poses within chain_compare.TAU; the local stage's reference is
                            re-evaluated from the device's Tcw_init where its float rounding differs
  2 gates leave alone       SKIPPED / BOW_FAILED: state, Tcw_init, n_edges[1], the pose status, the search's ops
  3 it is its parts         the composites against the calls they are made of, and the OK stage against the host-gated sequence of public calls
  4 the chain closes        frame_result into hs_keyframe_gate_device with ok_override = -1
  5 work area               exactly hs_track_initial_work_bytes behind guards, at both kf_caps
  6 old contents            five fills of outputs and work, two of them with hs_debug_poison on
  7 stream order            tests/stream_order.py: held-back stream, late inputs, early snapshots
  8 refusals                HS_ERR_INVALID and untouched outputs
  9 python methods          FrameTracker.TrackNormal / InitialPoseEstimation return what the raw call computed
The vocabulary goes through hs_vocab_from_tree + hs_vocab_upload; the store's node / weight are hs_bow_transform_device's.  Every device output has
guard bytes behind it, checked on every read."""
import ctypes as C

import numpy as np
import pytest

import devbuf
import hipmem
import ref_bow
import ref_refkf as RR
import ref_track as R
import refkf_cases as RC
import scenes
import stream_order as SO
from chain_compare import compare_stage

pytestmark = pytest.mark.gpu

GUARD = devbuf.GUARD
FILLS = (0x55, 0x00, 0xFF, 0xA5, 0xAA)         # tests/test_gpu_chain_run.py's four and 0xAA
TABLE_KEYS = ("lm_obs_offsets", "lm_obs_kf", "lm_obs_octave", "lm_bad", "lm_nobs", "kf_bad", "kf_id")
STATE = ("kp_lm", "kp_outl", "n_matches")
# fields a stage defines completely, by the stage that writes them
INIT_WHOLE = ("bow_word", "bow_weight", "bow_node", "match_kf", "op_view", "op_lm", "pose_view", "problem", "n_edges", "pose", "Tcw_init", "result")
MOTION_WHOLE = ("last_lms", "narrow_idx", "narrow_dist", "narrow_n", "wide_idx", "wide_dist", "wide_n", "op_view", "n_edges_motion", "pose_motion")
LOCAL_WHOLE = ("n_edges_local", "pose_local", "local.weights", "local.max_slot", "local.max_count", "local.local", "local.n_local", "local.frame_remove", "local.sel",
               "local.n_sel", "local.lms", "local.match_idx", "local.match_dist", "local.n_matches")


@pytest.fixture(autouse=True)
def nothing_more_after_a_device_error(gpu):
    """a HIP error that a test left behind (a fault is sticky) ends the module's run: nothing more is started on that device"""
    yield
    rc = hipmem.hip().hipDeviceSynchronize()
    if rc != 0:
        pytest.exit("hipError %d after this test: nothing more is started on the device" % rc, returncode=3)


@pytest.fixture(scope="module")
def tracker(gpu):
    import hyslam_amd as HS
    return HS.FrameTracker(HS.ORBExtractor(device=0))


@pytest.fixture(scope="module")
def world(tracker):
    """the per-case device inputs (vocabulary, store, frame, tables), made once per case and shared by the tests"""
    w = World(tracker)
    yield w
    w.close()


# ---------------------------------------------------------------- buffers with a fill of the test's choice
def out_buf(nbytes, fill=devbuf.PATTERN):
    if fill == devbuf.PATTERN:
        return devbuf.out_buf(nbytes)
    b = hipmem.DevBuf(nbytes + GUARD)
    b.fill(fill)
    return b


def guarded(a, fill=devbuf.PATTERN):
    a = np.ascontiguousarray(a)
    b = out_buf(a.nbytes, fill)
    hipmem._ok(hipmem.hip().hipMemcpy(b.ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")
    return b


def read(buf, dtype, count, fill=devbuf.PATTERN):
    nbytes = np.dtype(dtype).itemsize * count
    raw = buf.to_numpy(np.uint8, nbytes + GUARD)
    assert (raw[nbytes:] == fill).all(), "bytes written behind the output"
    return raw[:nbytes].view(dtype).copy()


def put(buf, a):
    a = np.ascontiguousarray(a)
    hipmem._ok(hipmem.hip().hipMemcpy(buf.ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")


# ---------------------------------------------------------------- a case's inputs on the device
def upload_vocabulary(ex, tree, levelsup):
    """-> (DeviceVocabulary, the hs_vocab it was uploaded from): hs_vocab_from_tree, hs_vocab_get_tree, hs_vocab_upload"""
    from hyslam_amd import _native as N
    from hyslam_amd.distributed import DeviceVocabulary
    v, T = C.c_void_p(), N.VocabTree()
    assert ex._lib.hs_vocab_from_tree(C.byref(scenes.tree_struct(N.VocabTree, tree)), 3, C.byref(v)) == N.HS_OK
    assert ex._lib.hs_vocab_get_tree(v, C.byref(T)) == N.HS_OK
    return DeviceVocabulary(ex, T, levelsup), v


class Scene:
    """one case's inputs, resident: the vocabulary, the key-frame store with node / weight from hs_bow_transform_device, the frame, the map's tables,
    the last frame, the poses"""

    def __init__(self, tracker, c):
        from hyslam_amd import _native as N
        self.N, self.c = N, c
        ex, fr, K = tracker._ex, c["frame"], c["K"]
        self.n, self.n_last, self.L, self.cap, self.n_kf = len(fr["kps"]), len(c["last_kp_lm"]), len(c["lms"]), c["cap"], len(c["T"]["kf_id"])
        self.voc, self.v = upload_vocabulary(ex, c["tree"], c["levelsup"])
        total = len(K["kps"])
        self.kdesc = devbuf.dev(np.ascontiguousarray(K["desc"], np.uint8))
        self.k_out = [devbuf.out_buf(max(total, 1) * 4) for _ in range(3)]                                # word, weight, node of the whole store
        st = hipmem.Stream()
        self.voc.transform_device(self.kdesc.ptr, 0, total, self.k_out[0].ptr, self.k_out[1].ptr, self.k_out[2].ptr, st.ptr)
        st.synchronize()
        _, kwt, knd = ref_bow.bow_transform(c["tree"], K["desc"], c["levelsup"])
        assert np.array_equal(devbuf.read(self.k_out[2], np.int32, total), knd) and devbuf.read(self.k_out[1], np.float32, total).tobytes() == kwt.tobytes()
        assert np.array_equal(np.where(kwt > 0, knd, -1), K["node"])                                      # the case's masked nodes say the same
        self.kkeep = [devbuf.dev(np.ascontiguousarray(K["kf_off"], np.int64)), devbuf.dev(np.ascontiguousarray(K["kps"], N.KP_DTYPE)),
                      devbuf.dev(np.ascontiguousarray(K["kp_lm"], np.int32))]
        self.KF = N.KfFeatures(K["n_kf"], self.kkeep[0].ptr, self.kkeep[1].ptr, self.kdesc.ptr, self.k_out[2].ptr, self.kkeep[2].ptr, self.k_out[1].ptr)
        self.F = N.FrameView()
        F = self.F
        F.fx, F.fy, F.cx, F.cy, F.mbf, F.sensor = fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["mbf"], fr["sensor"]
        F.min_x, F.max_x, F.min_y, F.max_y = fr["bounds"]
        F.size_ref, F.n = 31.0, self.n
        self.fkeep = [devbuf.dev(np.ascontiguousarray(fr["kps"], N.KP_DTYPE)), devbuf.dev(np.ascontiguousarray(fr["desc"], np.uint8)),
                      devbuf.dev(np.ascontiguousarray(fr["uR"], np.float32))]
        F.kps, F.desc, F.uR = (b.ptr for b in self.fkeep)
        self.tkeep = [devbuf.dev(c["T"][k]) for k in TABLE_KEYS]
        self.KT = N.KfTable(self.L, self.n_kf, *[b.ptr for b in self.tkeep])
        self.d_lms = devbuf.dev(np.ascontiguousarray(c["lms"], N.LM_DTYPE))
        self.d_Tpred, self.d_Tlast, self.d_Tentry = (devbuf.dev(np.ascontiguousarray(c[k], np.float32)) for k in ("Tcw_pred", "Tcw_last", "Tcw_entry"))
        self.d_last_kps, self.d_last_kp_lm = devbuf.dev(np.ascontiguousarray(c["last_kps"], N.KP_DTYPE)), devbuf.dev(c["last_kp_lm"])
        self.d_neigh, self.d_parent, self.d_slot = devbuf.dev(c["neigh"]), devbuf.dev(c["parent"]), devbuf.dev(np.array([c["kf_slot"]], np.int32))
        tp, rp = c["tp"], c["rp"]
        self.tp = N.TrackParams(tp.th_motion, tp.th_motion_wide, tp.n_min_matches, tp.th_local, tp.nnratio_motion, tp.nnratio_local, tp.th_high, tp.sigma_ref,
                                tp.n_max_local_keyframes, tp.n_neighbor_keyframes)
        self.rp = N.TrackRefkfParams(rp.th_low, rp.nnratio, rp.n_min_matches_bow, rp.thresh_init)

    def close(self, ex):
        self.voc.close()
        ex._lib.hs_vocab_destroy(self.v)


class World:
    def __init__(self, tracker):
        self.tracker, self.scenes = tracker, {}

    def scene(self, c):
        if id(c) not in self.scenes:
            self.scenes[id(c)] = (Scene(self.tracker, c), c)
        return self.scenes[id(c)][0]

    def close(self):
        for s, _ in self.scenes.values():
            s.close(self.tracker._ex)


class Run:
    """one execution on a scene: the state, every output buffer and the work area behind guards of `fill`, a stream of its own"""

    def __init__(self, tracker, sc, fill=devbuf.PATTERN, kf_cap=None, state=None):
        N = sc.N
        self.N, self.tr, self.sc, self.fill = N, tracker, sc, fill
        c = sc.c
        self.kf_cap = c["kf_cap"] if kf_cap is None else kf_cap
        s0 = c["state0"] if state is None else state
        rng = np.random.default_rng(9)
        self.state = [guarded(s0[0], fill), guarded(s0[1], fill), guarded(np.array([s0[2]], np.int32), fill),
                      guarded(rng.integers(-1, 3, sc.n).astype(np.int32), fill)]                        # kp_lm_obs: dirty; the local stage rewrites it
        self.ST = N.TrackState(*[b.ptr for b in self.state])
        sizes = dict(n=sc.n, n_last=sc.n_last, n_kf=sc.n_kf, cap=sc.cap, kf_cap=self.kf_cap)
        self.spec = {}

        def alloc(spec, prefix=""):
            ptrs = []
            for k, kind, cnt in spec:
                dt, cnt = N.track_out_dtype(kind), sizes.get(cnt, cnt)
                self.spec[prefix + k] = (out_buf(dt.itemsize * cnt, fill), dt, cnt)
                ptrs.append(self.spec[prefix + k][0].ptr)
            return ptrs
        head, local, tail = alloc(N.TRACK_OUT_HEAD), alloc(N.LOCAL_MAP_OUT_SPEC, "local."), alloc(N.TRACK_OUT_TAIL)
        self.out = N.TrackOut(*head, N.LocalMapOut(*local), *tail)
        self.iout = N.TrackInitialOut(*alloc(N.TRACK_INITIAL_OUT_SPEC, "i."))
        self.work_bytes = tracker.track_initial_work_bytes(sc.n, sc.n_last, sc.L, sc.cap, self.kf_cap)
        self.work = out_buf(self.work_bytes, fill)
        self.stream = hipmem.Stream()

    def ptr(self, k, index=0):
        b, dt, _ = self.spec[k]
        return b.ptr + index * dt.itemsize

    # ---- the three entry points and the calls they are made of
    def _head(self, vv):
        sc = self.sc
        return (sc.F, vv, sc.d_Tpred.ptr, sc.d_last_kps.ptr, sc.d_last_kp_lm.ptr, sc.n_last, sc.voc._v, sc.KF, sc.d_slot.ptr, self.kf_cap, sc.d_Tlast.ptr,
                sc.d_Tentry.ptr, sc.KT, sc.d_lms.ptr)

    def normal(self, vv, stream=None):
        sc = self.sc
        self.tr.track_normal_device(*self._head(vv), sc.d_neigh.ptr, 10, sc.d_parent.ptr, sc.cap, sc.tp, sc.rp, self.ST, self.out, self.iout, self.work.ptr,
                                    stream or self.stream.ptr)

    def initial(self, vv):
        sc = self.sc
        self.tr.track_initial_device(*self._head(vv), sc.tp, sc.rp, self.ST, self.out, self.iout, self.work.ptr, self.stream.ptr)

    def motion(self):
        sc = self.sc
        self.tr.track_motion_model_device(sc.F, sc.d_Tpred.ptr, sc.d_last_kps.ptr, sc.d_last_kp_lm.ptr, sc.n_last, sc.KT, sc.d_lms.ptr, sc.tp, self.ST, self.out,
                                          self.work.ptr, self.stream.ptr)

    def refkf(self, vv):
        """hs_track_reference_keyframe_device as hs_track_initial_device calls it"""
        sc = self.sc
        entry = self.ptr("pose_motion") + self.N.POSE_RESULT_DTYPE.fields["Tcw"][1] if vv else sc.d_Tentry.ptr
        self.tr.track_reference_keyframe_device(sc.F, sc.voc._v, sc.KF, sc.d_slot.ptr, self.kf_cap, sc.d_Tlast.ptr, entry, self.ptr("result") if vv else None, sc.KT,
                                                sc.d_lms.ptr, sc.tp, sc.rp, self.ST, self.iout, self.work.ptr, self.stream.ptr)

    def local(self):
        sc = self.sc
        self.tr.track_local_map_device(sc.F, self.ptr("i.Tcw_init"), sc.KT, sc.d_lms.ptr, sc.d_neigh.ptr, 10, sc.d_parent.ptr, sc.cap, sc.tp, self.ST, self.out,
                                       self.work.ptr, self.stream.ptr)

    def host_gated(self, vv):
        """the stage from the existing public calls, the host reading the two gate words and doing what the gate kernels do (a case whose stage is OK)"""
        N, tr, ex, sc, c, s = self.N, self.tr, self.tr._ex, self.sc, self.sc.c, self.stream.ptr
        n, L, rp = sc.n, sc.L, c["rp"]
        if vv:                                                               # the first gate word: the motion stage's return value
            self.stream.synchronize()
            m = self.spec["result"][0].to_numpy(N.TRACK_RESULT_DTYPE, 1)[0]
            assert (-1 if int(m["status"]) == N.HS_TRACK_MOTION_FAILED else int(m["n_matches_map"])) < rp.thresh_init
        d_nbow = self.ptr("i.result") + N.TRACK_INITIAL_RESULT_DTYPE.fields["n_bow"][1]
        sc.voc.transform_device(sc.fkeep[1].ptr, 0, n, self.ptr("i.bow_word"), self.ptr("i.bow_weight"), self.ptr("i.bow_node"), s)
        tr.search_by_bow_kf_device(sc.KF, sc.d_slot.ptr, sc.KT, sc.fkeep[0].ptr, sc.fkeep[1].ptr, self.ptr("i.bow_node"), self.ptr("i.bow_weight"), n, rp.th_low, rp.nnratio,
                                   self.ptr("i.match_kf"), self.kf_cap, self.ptr("i.op_view"), self.ptr("i.op_lm"), d_nbow, None, s)
        self.stream.synchronize()
        n_bow = int(self.spec["i.result"][0].to_numpy(np.int32, 2)[1])                                    # the second gate word
        assert n_bow >= rp.n_min_matches_bow
        vassoc = out_buf(tr.track_refkf_work_bytes(n, 0, L))
        tr.frame_associate_views_device(n, L, self.state[0].ptr, self.state[1].ptr, self.state[2].ptr, self.ptr("i.op_view"), self.ptr("i.op_lm"), vassoc.ptr, s)
        tr.pose_views_device(sc.d_Tlast.ptr, self.ptr("i.pose_view"), s)
        prob = np.zeros(1, N.POSE_PROBLEM_DTYPE)
        prob["Tcw"][0] = np.asarray(c["Tcw_last"], np.float32).ravel()
        prob["fx"], prob["fy"], prob["cx"], prob["cy"], prob["bf"] = (c["frame"][k] for k in ("fx", "fy", "cx", "cy", "mbf"))
        self.stream.synchronize()
        put(self.spec["i.problem"][0], prob)
        Fs = N.FrameView.from_buffer_copy(sc.F)
        Fs.kp_lm_obs = self.state[3].ptr
        ex.pose_edges_device(Fs, sc.d_lms.ptr, L, self.state[0].ptr, self.ptr("i.edges"), n, self.ptr("i.n_edges", 0), c["tp"].sigma_ref, None, s)
        self.stream.synchronize()
        ne = self.spec["i.n_edges"][0].to_numpy(np.int32, 2)
        ne[1] = ne[0]
        put(self.spec["i.n_edges"][0], ne)
        ex.pose_optimize_device(1, self.ptr("i.problem"), self.ptr("i.edges"), self.ptr("i.outlier"), self.ptr("i.pose"), None, self.ptr("i.n_edges", 1), n, None, s)
        tr.track_discard_device(N.HS_TRACK_MOTION, self.ptr("i.edges"), self.ptr("i.n_edges", 1), n, self.ptr("i.outlier"), self.ptr("i.pose"), sc.KT, c["frame"]["sensor"],
                                self.state[0].ptr, self.state[1].ptr, self.state[2].ptr,
                                self.ptr("i.result") + N.TRACK_INITIAL_RESULT_DTYPE.fields["n_matches_map_refkf"][1], s)
        self.stream.synchronize()
        read(vassoc, np.uint8, tr.track_refkf_work_bytes(n, 0, L))

    def results(self):
        self.stream.synchronize()
        read(self.work, np.uint8, self.work_bytes, self.fill)
        got = {k: read(b, dt, cnt, self.fill) for k, (b, dt, cnt) in self.spec.items()}
        got["kp_lm"], got["kp_outl"] = read(self.state[0], np.int32, self.sc.n, self.fill), read(self.state[1], np.uint8, self.sc.n, self.fill)
        got["n_matches"], got["kp_lm_obs"] = read(self.state[2], np.int32, 1, self.fill), read(self.state[3], np.int32, self.sc.n, self.fill)
        return got


def defined(got, vv, local, frame_result=None):
    """-> {name: bytes}: every byte the calls define (edge and flag arrays up to their counts), for a run of the motion stage (vv), the initial stage
    and the local stage (local); frame_result: hs_track_normal_device ran (default: with the local stage)"""
    out = {"i." + k: got["i." + k].tobytes() for k in INIT_WHOLE}
    out.update({k: got[k].tobytes() for k in STATE})
    ne = got["i.n_edges"]
    out["i.edges"] = got["i.edges"][:ne[0]].tobytes()
    if ne[1] >= 3:
        out["i.outlier"] = got["i.outlier"][:ne[1]].tobytes()
    if vv:
        out.update({k: got[k].tobytes() for k in MOTION_WHOLE})
        out["pose_view0"], out["problem0"] = got["pose_view"][0].tobytes(), got["problem"][0].tobytes()
        out["edges_motion"] = got["edges_motion"][:got["n_edges_motion"][0]].tobytes()
        if got["n_edges_motion"][1] >= 3:
            out["outlier_motion"] = got["outlier_motion"][:got["n_edges_motion"][1]].tobytes()
        r = got["result"][0]
        out["result.motion"] = np.array([r[k] for k in ("status", "used_wide", "n_narrow", "n_wide", "n_matches_map")], np.int32).tobytes()
        if local:
            out["result"] = got["result"].tobytes()                                                       # motion zeroes the rest, local adds n_inliers
    if local:
        out.update({k: got[k].tobytes() for k in LOCAL_WHOLE})
        out["pose_view1"], out["problem1"], out["kp_lm_obs"] = got["pose_view"][1].tobytes(), got["problem"][1].tobytes(), got["kp_lm_obs"].tobytes()
        out["n_inliers"] = np.int32(got["result"][0]["n_inliers"]).tobytes()
        nl = int(got["n_edges_local"][0])
        out["edges_local"] = got["edges_local"][:nl].tobytes()
        if nl >= 3:
            out["outlier_local"] = got["outlier_local"][:nl].tobytes()
    if local if frame_result is None else frame_result:
        out["i.frame_result"] = got["i.frame_result"].tobytes()
    return out


def assert_same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert a[k] == b[k], (what, k)


# ---------------------------------------------------------------- 1: against the reference
def compare_initial(got, c, vv, ref, report, LM_DTYPE):
    """every output of hs_track_normal_device against the dense reference chain -> the local stage's reference that held (re-evaluated from the device's
    Tcw_init where the float poses differ)"""
    motion, rk, local = ref
    g = lambda k: got["i." + k]
    # the motion stage (tests/chain_compare.compare_track's first half)
    if vv:
        assert got["pose_view"][0].tobytes() == motion["pose_view"].tobytes()
        assert got["last_lms"].tobytes() == np.ascontiguousarray(motion["last_lms"], LM_DTYPE).tobytes()
        for k in ("narrow_idx", "narrow_dist", "wide_idx", "wide_dist", "op_view"):
            assert got[k].tobytes() == motion[k].tobytes(), (report, k)
        r = got["result"][0]
        assert (int(r["status"]), int(r["used_wide"]), int(r["n_narrow"]), int(r["n_wide"]), int(r["n_matches_map"])) == \
            (motion["status"], motion["used_wide"], motion["narrow_n"], motion["wide_n"], motion["n_matches_map"]), report
        assert got["n_edges_motion"].tolist() == [motion["n_edges"], motion["n_edges_run"]]
        compare_stage(got, motion, "motion", c, report)
    # the transform and the search: they run in every case
    assert np.array_equal(g("bow_word"), rk["bow_word"]) and np.array_equal(g("bow_node"), rk["bow_node"]), report
    assert g("bow_weight").tobytes() == np.ascontiguousarray(rk["bow_weight"], np.float32).tobytes(), report
    for k in ("match_kf", "op_view", "op_lm"):
        assert np.array_equal(g(k), rk[k]), (report, k)
    assert g("n_edges").tolist() == [int(v) for v in rk["n_edges"]], (report, g("n_edges"), rk["n_edges"])
    assert g("pose_view")[0].tobytes() == R.pose_view(c["Tcw_last"]).tobytes(), report
    # the optimiser: compare_stage on the stage's own names
    stage = dict(n_edges=int(rk["n_edges"][0]), edges=rk["edges"], pose=rk["pose"])
    same = compare_stage({"pose_refkf": g("pose"), "n_edges_refkf": g("n_edges"), "edges_refkf": g("edges"), "outlier_refkf": g("outlier")}, stage, "refkf", c, report)
    assert g("result").tobytes() == rk["result"].tobytes(), (report, g("result"), rk["result"])
    ok = rk["status"] == RR.REFKF_OK
    # Tcw_init: the optimiser's float pose, or the entry pose: the device's own bytes, which compare_stage held within TAU of the reference's
    entry = got["pose_motion"][0]["Tcw"] if vv else np.asarray(c["Tcw_entry"], np.float32).reshape(16)
    assert g("Tcw_init").tobytes() == (g("pose")[0]["Tcw"] if ok else entry).tobytes(), report
    ulps = np.abs(g("Tcw_init").view(np.int32).astype(np.int64) - np.ascontiguousarray(rk["Tcw_init"], np.float32).view(np.int32).astype(np.int64))
    assert ulps.max() <= 1, report                                           # the float rounding of two doubles within TAU of each other
    if g("Tcw_init").tobytes() != np.ascontiguousarray(rk["Tcw_init"], np.float32).tobytes():
        print(report + ": the device's float pose differs from the reference's; the local stage is compared from the device's pose")
        _, rk2, local = RR.track_normal_dense(c, vv, c["state0"], Tcw_init=g("Tcw_init"))
        assert rk2["result"].tobytes() == rk["result"].tobytes()
    # (the state after the initial stage is checked by the runs that stop there: test_it_is_its_parts compares them with this run's parts)
    assert got["pose_view"][1].tobytes() == local["pose_view"].tobytes(), report
    for k in ("weights", "local", "frame_remove", "sel", "match_idx", "match_dist"):
        assert np.array_equal(got["local." + k], local[k]), (report, k)
    assert (int(got["local.max_slot"][0]), int(got["local.max_count"][0]), int(got["local.n_local"][0]), int(got["local.n_sel"][0]), int(got["local.n_matches"][0])) == \
        (local["max_slot"], local["max_count"], local["n_local"], local["n_sel"], local["n_matches"]), report
    assert got["local.lms"].tobytes() == np.ascontiguousarray(local["lms"], LM_DTYPE).tobytes(), report
    compare_stage(got, local, "local", c, report)
    assert int(got["result"][0]["n_inliers"]) == local["n_inliers"], report
    for gk, w, what in zip((got["kp_lm"], got["kp_outl"], int(got["n_matches"][0])), local["state"], STATE):
        assert np.array_equal(gk, w), (report, what)
    fr = got["i.frame_result"][0]
    want = (0, motion["used_wide"], motion["narrow_n"], motion["wide_n"]) if vv else (0, 0, 0, 0)
    assert (int(fr["status"]), int(fr["used_wide"]), int(fr["n_narrow"]), int(fr["n_wide"])) == want, report
    assert (int(fr["n_matches_map"]), int(fr["n_inliers"]), fr["_pad"].tolist()) == (int(rk["result"]["n_init"][0]), local["n_inliers"], [0, 0]), report
    return local


def initial_state(world, tracker, c, vv):
    """hs_track_initial_device alone -> its outputs and the state it leaves"""
    run = Run(tracker, world.scene(c))
    run.initial(vv)
    return run.results()


def check_case(world, tracker, c, vv, ref, report):
    run = Run(tracker, world.scene(c))
    run.normal(vv)
    got = run.results()
    local = compare_initial(got, c, vv, ref, report, run.N.LM_DTYPE)
    mid = initial_state(world, tracker, c, vv)                                # the three state arrays after the initial stage
    for k, w in zip(STATE, ref[1]["state"]):
        assert np.array_equal(mid[k] if k != "n_matches" else int(mid[k][0]), w), (report, "after the initial stage", k)
    return got, local, mid


@pytest.mark.parametrize("name", list(RC.DIRECTED))
def test_against_the_reference_directed(world, tracker, name):
    c, vv, ref = RC.directed(name)
    check_case(world, tracker, c, vv, ref, name)


def test_against_the_reference_random(world, tracker):
    cases, drawn = RC.random_cases()
    assert len(cases) == RC.N_RANDOM
    statuses = set()
    for c, vv, ref in cases:
        check_case(world, tracker, c, vv, ref, "seed %d" % c["seed"])
        statuses.add((vv, int(ref[1]["status"])))
    assert {(0, RR.REFKF_OK), (1, RR.REFKF_OK), (1, RR.REFKF_SKIPPED)} <= statuses


# ---------------------------------------------------------------- 2: gates leave things alone
GATED = ["bow_gate_below", "bow_gate_below_after_motion", "motion_gate_exact", "skipped", "slot_minus_one", "slot_past_the_store", "empty_keyframe"]
OK_CASES = [k for k in RC.DIRECTED if k not in GATED]


@pytest.mark.parametrize("name", GATED)
def test_gates_leave_things_alone(world, tracker, name):
    c, vv, (motion, rk, _) = RC.directed(name)
    assert rk["status"] != RR.REFKF_OK
    N = world.scene(c).N
    got = initial_state(world, tracker, c, vv)
    if vv:                                                                   # the state before the fall-back: the motion stage's, from the device itself
        before = Run(tracker, world.scene(c))
        before.motion()
        b = before.results()
        entry = b["pose_motion"][0]["Tcw"]
        for k, w in zip(STATE, motion["state"]):
            assert np.array_equal(b[k] if k != "n_matches" else int(b[k][0]), w), (name, k)
    else:
        b = dict(kp_lm=c["state0"][0], kp_outl=c["state0"][1], n_matches=np.array([c["state0"][2]], np.int32))
        entry = np.asarray(c["Tcw_entry"], np.float32).reshape(16)
    for k in STATE:
        assert got[k].tobytes() == np.ascontiguousarray(b[k]).tobytes(), (name, k)
    assert got["i.Tcw_init"].tobytes() == np.ascontiguousarray(entry).tobytes(), name
    assert int(got["i.n_edges"][1]) == 0 and int(got["i.pose"][0]["status"]) == 1, name                 # HS_POSE_TOO_FEW
    assert got["i.pose"][0]["Tcw"].tobytes() == np.asarray(c["Tcw_last"], np.float32).tobytes(), name
    assert np.array_equal(got["i.op_view"], rk["op_view"]) and np.array_equal(got["i.op_lm"], rk["op_lm"]), name
    if rk["status"] == RR.REFKF_SKIPPED:
        assert (rk["op_view"] >= 0).any(), name                              # ... and there was something to mask
    r = got["i.result"][0]
    assert int(r["refkf_status"]) == rk["status"] and int(r["n_matches_map_refkf"]) == 0, name
    assert N.HS_REFKF_SKIPPED == RR.REFKF_SKIPPED


def test_the_gated_cases_are_every_gated_directed_case():
    st = {k: int(RC.directed(k)[2][1]["status"]) for k in RC.DIRECTED}
    assert sorted(k for k in st if st[k] != RR.REFKF_OK) == sorted(GATED)
    assert list(st.values()).count(RR.REFKF_SKIPPED) >= 2 and list(st.values()).count(RR.REFKF_BOW_FAILED) >= 4


# ---------------------------------------------------------------- 3: it is its parts
@pytest.mark.parametrize("name", ["plain", "bow_gate_below", "bow_gate_below_after_motion", "motion_gate_exact", "motion_gate_below", "fallback_after_weak_motion",
                                  "fallback_after_failed_motion", "skipped", "too_few_edges", "mono"])
def test_it_is_its_parts(world, tracker, name):
    c, vv, _ = RC.directed(name)
    sc = world.scene(c)
    whole, parts = Run(tracker, sc), Run(tracker, sc)
    whole.initial(vv)
    if vv:
        parts.motion()
    parts.refkf(vv)
    assert_same(defined(whole.results(), vv, False), defined(parts.results(), vv, False), (name, "hs_track_initial_device"))
    whole, parts = Run(tracker, sc), Run(tracker, sc)
    whole.normal(vv)
    if vv:
        parts.motion()
    parts.refkf(vv)
    parts.local()
    assert_same(defined(whole.results(), vv, True, frame_result=False), defined(parts.results(), vv, True, frame_result=False), (name, "hs_track_normal_device"))


@pytest.mark.parametrize("name", OK_CASES)
def test_the_stage_is_the_host_gated_sequence(world, tracker, name):
    """on the cases whose stage runs: hs_track_reference_keyframe_device against the existing public calls made one by one, the host reading the two gate
    words (behind the motion stage where the velocity is valid)"""
    c, vv, (_, rk, _) = RC.directed(name)
    assert rk["status"] == RR.REFKF_OK
    sc = world.scene(c)
    one, apart = Run(tracker, sc), Run(tracker, sc)
    if vv:
        one.motion(), apart.motion()
    one.refkf(vv)
    apart.host_gated(vv)
    a, b = defined(one.results(), vv, False), defined(apart.results(), vv, False)
    ra, rb = np.frombuffer(a.pop("i.result"), np.int32), np.frombuffer(b.pop("i.result"), np.int32)
    assert (ra[1], ra[2]) == (rb[1], rb[2]), name                            # n_bow and the discard's count: the two words both write
    a.pop("i.Tcw_init"), b.pop("i.Tcw_init")
    assert_same(a, b, (name, "host-gated"))
    assert one.results()["i.Tcw_init"].tobytes() == apart.results()["i.pose"][0]["Tcw"].tobytes()


# ---------------------------------------------------------------- 4: the chain closes
@pytest.mark.parametrize("name", list(RC.DIRECTED))
def test_the_chain_closes(world, tracker, name):
    """frame_result into hs_keyframe_gate_device with ok_override = -1: ok = success && n_inliers > thresh_refine, at a threshold the frame passes, at
    n_inliers itself (the comparison is strict) and one below"""
    c, vv, ref = RC.directed(name)
    N = world.scene(c).N
    run = Run(tracker, world.scene(c))
    run.normal(vv)
    got = run.results()
    success, n_inl = int(ref[1]["result"]["success"][0]), int(got["result"][0]["n_inliers"])
    assert int(got["i.result"][0]["success"]) == success
    local = ref[2]
    if got["i.Tcw_init"].tobytes() != np.ascontiguousarray(ref[1]["Tcw_init"], np.float32).tobytes():
        local = RR.track_normal_dense(c, vv, c["state0"], Tcw_init=got["i.Tcw_init"])[2]
    assert n_inl == local["n_inliers"]
    d_res = devbuf.out_buf(N.KEYFRAME_RESULT_DTYPE.itemsize)
    for thresh_refine in (30, n_inl, n_inl - 1):
        prm = N.KeyFrameParams(thresh_init=c["rp"].thresh_init, thresh_refine=thresh_refine, ok_override=-1)
        tracker.keyframe_gate_device(run.ptr("i.frame_result"), prm, d_res.ptr, run.stream.ptr)
        run.stream.synchronize()
        ok = int(devbuf.read(d_res, N.KEYFRAME_RESULT_DTYPE, 1)[0]["ok"])
        assert ok == int(bool(success) and local["n_inliers"] > thresh_refine), (name, thresh_refine, ok)
    if name == "fallback_after_failed_motion":                               # the motion stage's own record says MOTION_FAILED: the old gate would say 0
        assert int(got["result"][0]["status"]) == N.HS_TRACK_MOTION_FAILED and success == 1
        prm = N.KeyFrameParams(thresh_init=c["rp"].thresh_init, thresh_refine=30, ok_override=-1)
        tracker.keyframe_gate_device(run.ptr("result"), prm, d_res.ptr, run.stream.ptr)
        run.stream.synchronize()
        assert int(devbuf.read(d_res, N.KEYFRAME_RESULT_DTYPE, 1)[0]["ok"]) == 0


# ---------------------------------------------------------------- 5: the work area
@pytest.mark.parametrize("name,kf_cap", [("plain", 80), ("kf_cap_truncates", 50), ("fallback_after_weak_motion", 80), ("fallback_after_weak_motion", 50)])
def test_work_area_is_exactly_its_size(world, tracker, name, kf_cap):
    """d_work is hs_track_initial_work_bytes and not a byte more (Run.results reads the guard behind it and behind every output); the work area's old
    contents do not matter: the same bytes from a block of another fill; at kf_cap 50 the key frame of 80 is truncated"""
    c, vv, ref = RC.directed(name)
    sc = world.scene(c)
    runs = [Run(tracker, sc, kf_cap=kf_cap), Run(tracker, sc, kf_cap=kf_cap, fill=0xC3)]
    assert runs[0].work_bytes == tracker.track_initial_work_bytes(sc.n, sc.n_last, sc.L, sc.cap, kf_cap) >= \
        tracker.track_work_bytes(sc.n, sc.n_last, sc.L, sc.cap) + tracker.track_refkf_work_bytes(sc.n, 0, sc.L) + 8 * sc.n
    for r in runs:
        r.normal(vv)
    a, b = (defined(r.results(), vv, True) for r in runs)
    assert_same(a, b, (name, kf_cap))
    got = runs[0].results()
    want = RR.search_by_bow_kf_dense(c["K"], c["kf_slot"], kf_cap, sc.L, c["T"]["lm_bad"], c["frame"]["kps"], c["frame"]["desc"], ref[1]["bow_node"], ref[1]["bow_weight"],
                                     c["rp"].th_low, c["rp"].nnratio)
    assert np.array_equal(got["i.match_kf"], want[0]) and int(got["i.result"][0]["n_bow"]) == want[3], (name, kf_cap)
    if kf_cap == c["kf_cap"]:
        assert got["i.result"].tobytes() == ref[1]["result"].tobytes()


# ---------------------------------------------------------------- 6: no dependence on old contents
@pytest.mark.parametrize("name", ["fallback_after_weak_motion", "skipped", "bow_gate_below"])
def test_results_do_not_depend_on_old_contents(world, tracker, name):
    """one OK, one SKIPPED, one BOW_FAILED case; outputs, state guards and work pre-filled with five bytes, two of the runs with hs_debug_poison on (the
    library's own arena then carries the byte too): every defined byte identical"""
    c, vv, ref = RC.directed(name)
    assert int(ref[1]["status"]) == dict(fallback_after_weak_motion=RR.REFKF_OK, skipped=RR.REFKF_SKIPPED, bow_gate_below=RR.REFKF_BOW_FAILED)[name]
    lib, sc, seen = tracker._ex._lib, world.scene(c), []
    before = lib.hs_debug_poison_violations()
    try:
        for fill in FILLS:
            if fill in (0x00, 0xFF):
                assert lib.hs_debug_poison(fill) == 0
            run = Run(tracker, sc, fill=fill)
            run.normal(vv)
            seen.append(defined(run.results(), vv, True))
            lib.hs_debug_poison(-1)
    finally:
        lib.hs_debug_poison(-1)
    assert lib.hs_debug_poison_violations() == before
    for k in range(1, len(FILLS)):
        assert_same(seen[0], seen[k], (name, hex(FILLS[k])))
    assert np.frombuffer(seen[0]["i.result"], RR.INIT_RESULT_DTYPE).tobytes() == ref[1]["result"].tobytes()


# ---------------------------------------------------------------- 7: stream order
def _same_tree(tree):
    def edit(c, rng):                                                        # the decoy lives under the real case's vocabulary: the store's nodes again
        RC._weak_motion(c, rng)
        c["tree"] = tree
        _, wt, nd = ref_bow.bow_transform(tree, c["K"]["desc"], c["levelsup"])
        c["K"]["node"] = np.where(wt > 0, nd, -1).astype(np.int32)
    return edit


def stream_cases():
    """-> (real, decoy): (case, reference); the decoy is another seed of the same builder and edit"""
    real, vv, ref = RC.directed("fallback_after_weak_motion")
    decoy = RC.build(real["seed"] + 501, edit=_same_tree(real["tree"]))        # (its result record differs from the real case's in four words)
    return (real, ref), (decoy, RC.reference(decoy, 1))


def stream_step(tracker, voc, N, real, decoy):
    (c, ref), (d, dref) = real, decoy
    n, n_last, L, n_kf, cap, kf_cap = RC.N, RC.N_LAST, len(c["lms"]), len(c["T"]["kf_id"]), c["cap"], c["kf_cap"]
    assert (len(d["lms"]), d["cap"], d["kf_cap"], len(d["K"]["kps"])) == (L, cap, kf_cap, len(c["K"]["kps"]))

    def arrays(x):
        K, fr = x["K"], x["frame"]
        _, kwt, knd = ref_bow.bow_transform(x["tree"], K["desc"], x["levelsup"])
        a = {"F.kps": np.ascontiguousarray(fr["kps"], N.KP_DTYPE), "F.desc": np.ascontiguousarray(fr["desc"], np.uint8), "F.uR": np.ascontiguousarray(fr["uR"], np.float32),
             "K.kf_off": np.ascontiguousarray(K["kf_off"], np.int64), "K.kps": np.ascontiguousarray(K["kps"], N.KP_DTYPE), "K.desc": np.ascontiguousarray(K["desc"], np.uint8),
             "K.node": np.ascontiguousarray(knd, np.int32), "K.kp_lm": np.ascontiguousarray(K["kp_lm"], np.int32), "K.weight": np.ascontiguousarray(kwt, np.float32),
             "lms": np.ascontiguousarray(x["lms"], N.LM_DTYPE), "Tpred": np.ascontiguousarray(x["Tcw_pred"], np.float32), "Tlast": np.ascontiguousarray(x["Tcw_last"], np.float32),
             "Tentry": np.ascontiguousarray(x["Tcw_entry"], np.float32), "last_kps": np.ascontiguousarray(x["last_kps"], N.KP_DTYPE),
             "last_kp_lm": np.ascontiguousarray(x["last_kp_lm"], np.int32), "neigh": np.ascontiguousarray(x["neigh"], np.int32),
             "parent": np.ascontiguousarray(x["parent"], np.int32), "slot": np.array([x["kf_slot"]], np.int32)}
        a.update({"T." + k: np.ascontiguousarray(x["T"][k]) for k in TABLE_KEYS})
        return a
    ra, da = arrays(c), arrays(d)
    for k in ("T.lm_obs_kf", "T.lm_obs_octave"):                             # the observation lists' lengths are the seeds' own: padded behind offsets[-1]
        m = max(len(ra[k]), len(da[k]))
        ra[k], da[k] = (np.concatenate([a[k], np.zeros(m - len(a[k]), a[k].dtype)]) for a in (ra, da))
    inputs = {k: (ra[k], da[k]) for k in ra}
    sizes = dict(n=n, n_last=n_last, n_kf=n_kf, cap=cap, kf_cap=kf_cap)
    outputs, dts = {}, {}
    for prefix, spec in (("", N.TRACK_OUT_HEAD), ("local.", N.LOCAL_MAP_OUT_SPEC), ("", N.TRACK_OUT_TAIL), ("i.", N.TRACK_INITIAL_OUT_SPEC)):
        for k, kind, cnt in spec:
            dts[prefix + k] = (N.track_out_dtype(kind), sizes.get(cnt, cnt))
            outputs[prefix + k] = dts[prefix + k][0].itemsize * dts[prefix + k][1]
    outputs.update(kp_lm=4 * n, kp_outl=n, n_matches=4, kp_lm_obs=4 * n)      # the motion stage clears the state first: an output
    dts.update(kp_lm=(np.dtype(np.int32), n), kp_outl=(np.dtype(np.uint8), n), n_matches=(np.dtype(np.int32), 1), kp_lm_obs=(np.dtype(np.int32), n))
    work = dict(work=tracker.track_initial_work_bytes(n, n_last, L, cap, kf_cap))
    tp, rp = c["tp"], c["rp"]
    TP = N.TrackParams(tp.th_motion, tp.th_motion_wide, tp.n_min_matches, tp.th_local, tp.nnratio_motion, tp.nnratio_local, tp.th_high, tp.sigma_ref,
                       tp.n_max_local_keyframes, tp.n_neighbor_keyframes)
    RP = N.TrackRefkfParams(rp.th_low, rp.nnratio, rp.n_min_matches_bow, rp.thresh_init)
    fr = c["frame"]
    assert all(fr[k] == d["frame"][k] for k in ("fx", "fy", "cx", "cy", "mbf", "sensor", "bounds")) and (d["rp"].thresh_init, d["kf_slot"]) == (rp.thresh_init, c["kf_slot"])

    def call(p, s):
        F = N.FrameView()
        F.fx, F.fy, F.cx, F.cy, F.mbf, F.sensor = fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["mbf"], fr["sensor"]
        F.min_x, F.max_x, F.min_y, F.max_y = fr["bounds"]
        F.size_ref, F.n = 31.0, n
        F.kps, F.desc, F.uR = p["F.kps"], p["F.desc"], p["F.uR"]
        KF = N.KfFeatures(c["K"]["n_kf"], p["K.kf_off"], p["K.kps"], p["K.desc"], p["K.node"], p["K.kp_lm"], p["K.weight"])
        KT = N.KfTable(L, n_kf, *[p["T." + k] for k in TABLE_KEYS])
        ST = N.TrackState(p["kp_lm"], p["kp_outl"], p["n_matches"], p["kp_lm_obs"])
        out = N.TrackOut(*[p[k] for k, _, _ in N.TRACK_OUT_HEAD], N.LocalMapOut(*[p["local." + k] for k, _, _ in N.LOCAL_MAP_OUT_SPEC]), *[p[k] for k, _, _ in N.TRACK_OUT_TAIL])
        iout = N.TrackInitialOut(*[p["i." + k] for k, _, _ in N.TRACK_INITIAL_OUT_SPEC])
        tracker.track_normal_device(F, 1, p["Tpred"], p["last_kps"], p["last_kp_lm"], n_last, voc._v, KF, p["slot"], kf_cap, p["Tlast"], p["Tentry"], KT, p["lms"], p["neigh"], 10,
                                    p["parent"], cap, TP, RP, ST, out, iout, p["work"], s)

    def exact(x):                                                            # the integer outputs the reference gives in full, whatever the float rounding
        m, rk, _ = x
        return {"i.bow_word": rk["bow_word"], "i.bow_node": rk["bow_node"], "i.bow_weight": np.ascontiguousarray(rk["bow_weight"], np.float32), "i.match_kf": rk["match_kf"],
                "i.op_view": rk["op_view"], "i.op_lm": rk["op_lm"], "i.n_edges": np.array(rk["n_edges"], np.int32), "i.result": rk["result"],
                "narrow_idx": m["narrow_idx"], "wide_idx": m["wide_idx"], "op_view": m["op_view"], "n_edges_motion": np.array([m["n_edges"], m["n_edges_run"]], np.int32)}
    er, ed = exact(ref), exact(dref)
    expect = {k: [(0, np.ascontiguousarray(er[k]), np.ascontiguousarray(ed[k]))] for k in er}

    def check(got, which):
        g = {k: got[k].view(dts[k][0])[:dts[k][1]] for k in outputs}
        compare_initial(g, c, 1, ref, "stream order", N.LM_DTYPE)
    return SO.Step("hs_track_normal_device", inputs, outputs, call, expect, work=work, check=check)


def test_stream_order(world, tracker, gpu):
    import hyslam_amd as HS
    from hyslam_amd import _native as N
    real, decoy = stream_cases()
    assert int(real[1][1]["status"]) == RR.REFKF_OK and real[1][1]["result"].tobytes() != decoy[1][1]["result"].tobytes()
    voc = world.scene(real[0]).voc
    delay_ex = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=500), device=0)               # the delay's handle: never the handle under test
    # one call outside the harness first, on the decoy in buffers of its own: the projection searches' grid lists come from the handle's scratch, which
    # must not grow (and drain the stream) under the delay
    st, s0 = stream_step(tracker, voc, N, real, decoy), hipmem.Stream()
    bufs = {k: hipmem.DevBuf.from_numpy(SO._raw(dd)) for k, (r, dd) in st.inputs.items()}
    bufs.update({k: hipmem.DevBuf(nb) for k, nb in list(st.outputs.items()) + list(st.work.items())})
    st.call({k: b.ptr for k, b in bufs.items()}, s0.ptr)
    s0.synchronize()
    for i, (steps, got, after) in enumerate(SO.run(delay_ex, lambda: [stream_step(tracker, voc, N, real, decoy)], tag="hs_track_normal_device")):
        SO.check(steps, got, after, "hs_track_normal_device [caller stream %d]" % i)
    delay_ex.close()


# ---------------------------------------------------------------- 8: refusals
def test_refusals(world, tracker):
    """what the three entry points refuse on the host, before the first launch: each gives HS_ERR_INVALID and every output, the state and the work area
    keep their bytes"""
    from hyslam_amd import _native as N
    c, vv, ref = RC.directed("fallback_after_weak_motion")
    sc, lib, h = world.scene(c), tracker._ex._lib, tracker._ex._h
    run = Run(tracker, sc)

    def args(**kw):
        a = dict(F=sc.F, vv=1, Tpred=sc.d_Tpred.ptr, last_kps=sc.d_last_kps.ptr, last_kp_lm=sc.d_last_kp_lm.ptr, n_last=sc.n_last, voc=sc.voc._v, K=sc.KF, slot=sc.d_slot.ptr,
                 kf_cap=run.kf_cap, Tlast=sc.d_Tlast.ptr, Tentry=sc.d_Tentry.ptr, T=sc.KT, lms=sc.d_lms.ptr, neigh=sc.d_neigh.ptr, parent=sc.d_parent.ptr, cap=sc.cap,
                 tp=sc.tp, rp=sc.rp, st=run.ST, out=run.out, iout=run.iout, work=run.work.ptr, motion=run.ptr("result"))
        a.update(kw)
        return a
    ref_ = lambda v: None if v is None else C.byref(v)

    def normal(**kw):
        a = args(**kw)
        return lib.hs_track_normal_device(h, ref_(a["F"]), a["vv"], a["Tpred"], a["last_kps"], a["last_kp_lm"], a["n_last"], a["voc"], ref_(a["K"]), a["slot"], a["kf_cap"],
                                          a["Tlast"], a["Tentry"], ref_(a["T"]), a["lms"], a["neigh"], 10, a["parent"], a["cap"], ref_(a["tp"]), ref_(a["rp"]), ref_(a["st"]),
                                          ref_(a["out"]), ref_(a["iout"]), a["work"], run.stream.ptr)

    def initial(**kw):
        a = args(**kw)
        return lib.hs_track_initial_device(h, ref_(a["F"]), a["vv"], a["Tpred"], a["last_kps"], a["last_kp_lm"], a["n_last"], a["voc"], ref_(a["K"]), a["slot"], a["kf_cap"],
                                           a["Tlast"], a["Tentry"], ref_(a["T"]), a["lms"], ref_(a["tp"]), ref_(a["rp"]), ref_(a["st"]), ref_(a["out"]), ref_(a["iout"]),
                                           a["work"], run.stream.ptr)

    def refkf(**kw):
        a = args(**kw)
        return lib.hs_track_reference_keyframe_device(h, ref_(a["F"]), a["voc"], ref_(a["K"]), a["slot"], a["kf_cap"], a["Tlast"], a["Tentry"], a["motion"], ref_(a["T"]),
                                                      a["lms"], ref_(a["tp"]), ref_(a["rp"]), ref_(a["st"]), ref_(a["iout"]), a["work"], run.stream.ptr)

    def without(struct, field, value=None):
        s = type(struct).from_buffer_copy(struct)
        setattr(s, field, value)
        return s
    no_kps, no_n = without(sc.F, "kps"), without(sc.F, "n", 0)
    big_n = without(sc.F, "n", 65536)
    bad = [dict(voc=None), dict(K=None), dict(K=without(sc.KF, "node")), dict(slot=None), dict(Tlast=None), dict(iout=None), dict(work=None), dict(kf_cap=0), dict(kf_cap=-3),
           dict(F=no_n), dict(F=big_n), dict(F=no_kps), dict(F=None), dict(T=None), dict(T=without(sc.KT, "lm_bad")), dict(lms=None), dict(lms=sc.d_lms.ptr + 4),
           dict(tp=None), dict(rp=None), dict(st=None), dict(st=without(run.ST, "n_matches")), dict(iout=without(run.iout, "edges", run.ptr("i.edges") + 8))]
    bad += [dict(iout=without(run.iout, k)) for k, _, _ in N.TRACK_INITIAL_OUT_SPEC if k != "frame_result"]
    for kw in bad:
        for f in (normal, initial, refkf):
            assert f(**kw) == N.HS_ERR_INVALID, (f.__name__, list(kw))
    # what only some of them read
    assert normal(iout=without(run.iout, "frame_result")) == N.HS_ERR_INVALID and normal(cap=0) == N.HS_ERR_INVALID and normal(out=None) == N.HS_ERR_INVALID
    assert normal(iout=without(run.iout, "frame_result", run.ptr("result"))) == N.HS_ERR_INVALID
    assert initial(Tpred=None) == N.HS_ERR_INVALID and initial(out=None) == N.HS_ERR_INVALID and initial(n_last=0) == N.HS_ERR_INVALID
    assert initial(vv=0, Tentry=None) == N.HS_ERR_INVALID and normal(vv=0, Tentry=None) == N.HS_ERR_INVALID and refkf(Tentry=None) == N.HS_ERR_INVALID
    # what only the local stage reads, with and without a valid velocity: its outputs, neigh, parent; and what the projection searches of the motion and
    # local stages read: uR under a stereo sensor

    def out_without(field):
        o = type(run.out).from_buffer_copy(run.out)
        setattr(o.local, field, None)
        return o
    no_uR = without(sc.F, "uR")
    no_uR.sensor = no_uR.sensor or 1
    for vv in (1, 0):
        for kw in [dict(out=out_without(k)) for k, _, _ in N.LOCAL_MAP_OUT_SPEC] + [dict(neigh=None), dict(parent=None), dict(F=no_uR)]:
            assert normal(vv=vv, **kw) == N.HS_ERR_INVALID, ("normal", vv, list(kw))
    assert initial(F=no_uR) == N.HS_ERR_INVALID
    tracker._ex.synchronize()
    run.stream.synchronize()
    for k, (b, dt, cnt) in run.spec.items():
        assert (b.to_numpy(np.uint8, dt.itemsize * cnt + GUARD) == devbuf.PATTERN).all(), (k, "an output of a refused call was written")
    assert (run.work.to_numpy(np.uint8, run.work_bytes + GUARD) == devbuf.PATTERN).all()
    got = run.results()
    for k, w in zip(STATE, c["state0"]):
        assert np.array_equal(got[k] if k != "n_matches" else int(got[k][0]), w), k
    # the handle is as good as before; without a valid velocity the motion stage's arguments are not read
    run.normal(1)
    compare_initial(run.results(), c, 1, ref, "after the refusals", N.LM_DTYPE)
    c0, _, ref0 = RC.directed("plain")
    sc0 = world.scene(c0)
    r0 = Run(tracker, sc0)
    tracker.track_initial_device(sc0.F, 0, None, None, None, 0, sc0.voc._v, sc0.KF, sc0.d_slot.ptr, r0.kf_cap, sc0.d_Tlast.ptr, sc0.d_Tentry.ptr, sc0.KT, sc0.d_lms.ptr, sc0.tp,
                                 sc0.rp, r0.ST, None, r0.iout, r0.work.ptr, r0.stream.ptr)
    assert r0.results()["i.result"].tobytes() == ref0[1]["result"].tobytes()


# ---------------------------------------------------------------- 9: the python methods
@pytest.mark.parametrize("name", ["plain", "fallback_after_weak_motion", "skipped"])
def test_python_methods_return_what_the_raw_call_computed(world, tracker, name):
    c, vv, ref = RC.directed(name)
    sc = world.scene(c)
    run = Run(tracker, sc)
    run.normal(vv)
    got = run.results()
    kw = dict(Tcw_pred=c["Tcw_pred"], last_kps=c["last_kps"], last_kp_lm=c["last_kp_lm"]) if vv else dict(Tcw_entry=c["Tcw_entry"])
    res = tracker.TrackNormal(c["frame"], sc.voc, c["K"], c["kf_slot"], c["Tcw_last"], c["T"], c["lms"], c["neigh"], c["parent"], vv, state=c["state0"], params=sc.tp,
                              refkf_params=sc.rp, kf_cap=c["kf_cap"], cap=c["cap"], **kw)
    assert np.array_equal(res["kp_lm"], got["kp_lm"]) and np.array_equal(res["kp_outl"], got["kp_outl"]) and res["n_matches"] == int(got["n_matches"][0])
    r = got["i.result"][0]
    for k in ("refkf_status", "n_bow", "n_matches_map_refkf", "n_init", "success"):
        assert res[k] == int(r[k]), k
    assert res["Tcw_init"].tobytes() == got["i.Tcw_init"].tobytes() and res["pose_refkf"].tobytes() == got["i.pose"][0].tobytes()
    assert res["pose_local"].tobytes() == got["pose_local"][0].tobytes() and res["n_inliers"] == int(got["result"][0]["n_inliers"])
    assert res["frame_result"].tobytes() == got["i.frame_result"][0].tobytes()
    if vv:
        assert res["pose_motion"].tobytes() == got["pose_motion"][0].tobytes() and res["n_matches_map"] == int(got["result"][0]["n_matches_map"])
    # the initial stage through its own method leaves the state hs_track_initial_device leaves
    ini = tracker.InitialPoseEstimation(c["frame"], sc.voc, c["K"], c["kf_slot"], c["Tcw_last"], c["T"], c["lms"], vv, state=c["state0"], params=sc.tp, refkf_params=sc.rp,
                                        kf_cap=c["kf_cap"], **kw)
    for k, w in zip(STATE, ref[1]["state"]):
        assert np.array_equal(ini[k], w), k
    assert ini["n_init"] == res["n_init"] and ini["Tcw_init"].tobytes() == res["Tcw_init"].tobytes()
