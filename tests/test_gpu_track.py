"""GPU: the resident tracking chain (include/hyslam_amd.h, "frame tracking on resident tables") against tests/ref_track.py, which
tests/test_track_ref.py pins on the CPU.

  * hs_frame_associate_device against the sequential LandMarkMatches model: randomised states, sizes around the 64-lane wave, the 256-thread
    workgroup (HS_TRACK_BLOCK) and 1024; ops in shuffled array order; twice, same bytes
  * hs_pose_views_device: exact bytes against the gemm restatement, a NaN pose included
  * the posed search and the posed local map: byte-equal to the by-value entry points
  * hs_track_discard_device / hs_frame_views_device against numpy: both modes, both sensors, TOO_FEW, edge_cap truncation
  * hs_track_frame_device IS its parts: the two stage calls, and the public device calls made one by one with the host doing the glue
  * end to end against the reference on the directed and the random cases: every integer exactly, Tcw_d within tau
  * FrameTracker.TrackFrame returns the same
Every device output has guard bytes behind it, checked on every read."""
import ctypes as C

import numpy as np
import pytest

import hipmem
import ref_track as R
import track_cases as TC
from chain_compare import compare_track, same_outputs

pytestmark = pytest.mark.gpu

GUARD = 64
BLOCK = 256             # HS_TRACK_BLOCK


@pytest.fixture(scope="module")
def tracker(gpu):
    import hyslam_amd as HS
    return HS.FrameTracker(HS.ORBExtractor(device=0))


def dev(a):
    return hipmem.DevBuf.from_numpy(np.ascontiguousarray(a))


def out_buf(nbytes):
    b = hipmem.DevBuf(nbytes + GUARD)
    b.fill(0x55)
    return b


def guarded(a):
    """an in/out array with guard bytes behind it"""
    a = np.ascontiguousarray(a)
    b = out_buf(a.nbytes)
    hipmem._ok(hipmem.hip().hipMemcpy(b.ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")
    return b


def read(buf, dtype, count):
    nbytes = np.dtype(dtype).itemsize * count
    raw = buf.to_numpy(np.uint8, nbytes + GUARD)
    assert (raw[nbytes:] == 0x55).all(), "bytes written behind the output"
    return raw[:nbytes].view(dtype).copy()


# ---------------------------------------------------------------- the replay
ASSOC_SIZES = [(1, 1), (1, 65), (63, 65), (64, 64), (65, 63), (130, 130), (100, 300), (BLOCK - 1, BLOCK + 1), (BLOCK, BLOCK), (BLOCK + 1, BLOCK - 1),
               (1023, 1025), (1024, 1024), (1025, 1023), (300, 1025), (1025, 1)]


def associate_device(tracker, s, order=None, stream=None):
    """stream: anything with .ptr and .synchronize() (default: a stream of its own)"""
    n, L = len(s["kp_lm"]), s["L"]
    ov, ol = (s["op_view"], s["op_lm"]) if order is None else (s["op_view"][order], s["op_lm"][order])
    d_lm, d_outl, d_nm = guarded(s["kp_lm"]), guarded(s["kp_outl"]), guarded(np.array([s["n_matches"]], np.int32))
    d_ov, d_ol = dev(ov), dev(ol)
    work = out_buf(tracker.track_work_bytes(n, 0, L, 0))
    st = stream or hipmem.Stream()
    tracker.frame_associate_device(n, L, d_lm.ptr, d_outl.ptr, d_nm.ptr, len(ov), d_ov.ptr, d_ol.ptr, work.ptr, st.ptr)
    st.synchronize()
    read(work, np.uint8, tracker.track_work_bytes(n, 0, L, 0))
    return read(d_lm, np.int32, n), read(d_outl, np.uint8, n), int(read(d_nm, np.int32, 1)[0])


@pytest.mark.parametrize("n,n_ops", ASSOC_SIZES)
def test_associate_against_the_sequential_model(tracker, n, n_ops):
    for seed in range(3):
        s = TC.replay_state(77000 + 1000 * seed + n, n, n_ops)
        want = R.replay_sequential(R.MapMatches.from_dense(s["kp_lm"], s["kp_outl"], s["n_matches"]), s["op_view"], s["op_lm"], n, s["L"]).dense(n)
        got = associate_device(tracker, s)
        for w, g, what in zip(want, got, ("kp_lm", "kp_outl", "n_matches")):
            assert np.array_equal(w, g), (what, n, n_ops, seed)
        again = associate_device(tracker, s, np.random.default_rng(seed).permutation(n_ops))       # array order does not matter, and the bytes repeat
        for a, g in zip(again, got):
            assert np.asarray(a).tobytes() == np.asarray(g).tobytes()


def test_associate_moves_a_landmark_and_keeps_a_stale_flag(tracker):
    """the path dependence, by hand: landmark 1 moves from view 0 to view 2 (n_matches unchanged, view 0's flag stays); landmark 3 lands on the empty
    view 3 whose stale `true` entry survives the fresh insert; landmark 0 then 2 hit view 1: the larger index stays, the flag is reset"""
    s = dict(kp_lm=np.array([1, -1, -1, -1], np.int32), kp_outl=np.array([2, 2, 0, 2], np.uint8), n_matches=1, L=4,
             op_view=np.array([1, 2, 1, 3], np.int32), op_lm=np.array([2, 1, 0, 3], np.int32))
    kp_lm, outl, nm = associate_device(tracker, s)
    assert kp_lm.tolist() == [-1, 2, 1, 3] and outl.tolist() == [2, 1, 1, 2] and nm == 3


# ---------------------------------------------------------------- the pose view
def test_pose_views_exact_bytes(tracker):
    poses, differs = [], 0
    for seed in range(24):
        rng = np.random.default_rng(seed)
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        T[:3, 3] = rng.normal(0, 3, 3)
        poses.append(T)
    nan = poses[0].copy(); nan[1, 3] = np.nan
    zero = np.zeros((4, 4), np.float32)                         # -1 * 0 + 0 = +0: the sign of cv::gemm's zero
    poses += [nan, zero]
    for T in poses:
        d_T, d_out = dev(T), out_buf(64)
        tracker.pose_views_device(d_T.ptr, d_out.ptr)
        tracker._ex.synchronize()
        got = read(d_out, np.uint8, 64)
        want = R.pose_view(T)
        assert got.tobytes() == want.tobytes(), (T, got.view(np.float32), want)
        differs += R.pose_view_float(T).tobytes() != want.tobytes()
    assert differs > 2                                          # poses on which a float accumulation gives other bytes are among them


# ---------------------------------------------------------------- posed entry points
def _device_frame(fa, pv=None):
    """-> (FrameView of device pointers, buffers); with pv the pose fields hold the pose view's values"""
    from hyslam_amd import _native as N
    F = N.FrameView()
    F.fx, F.fy, F.cx, F.cy, F.mbf, F.sensor = fa["fx"], fa["fy"], fa["cx"], fa["cy"], fa["mbf"], fa["sensor"]
    F.min_x, F.max_x, F.min_y, F.max_y = fa["bounds"]
    F.size_ref, F.n = 31.0, len(fa["kps"])
    bufs = [dev(np.ascontiguousarray(fa["kps"], N.KP_DTYPE)), dev(np.ascontiguousarray(fa["desc"], np.uint8)), dev(np.ascontiguousarray(fa["uR"], np.float32))]
    F.kps, F.desc, F.uR = (b.ptr for b in bufs)
    if fa.get("kp_lm_obs") is not None:
        bufs.append(dev(np.ascontiguousarray(fa["kp_lm_obs"], np.int32)))
        F.kp_lm_obs = bufs[-1].ptr
    if pv is not None:
        F.Rcw[:], F.tcw[:], F.Ow[:] = pv["Rcw"].tolist(), pv["tcw"].tolist(), pv["Ow"].tolist()
    return F, bufs


@pytest.mark.parametrize("criteria", [(1, 1, 0), (0, 1, 1)])
def test_posed_search_equals_the_search_by_value(tracker, criteria):
    """on the matcher tests' scene: the same outputs whether the kernel takes the pose from the launch arguments or from HBM"""
    import scenes
    from hyslam_amd import _native as N
    sc = scenes.projection_scene(71, 640, 480, nfeat=200, copies=3)
    fa, lms = sc["frame_args"], np.ascontiguousarray(sc["lms"], N.LM_DTYPE)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = fa["Rcw"], fa["tcw"]
    pv = R.pose_view(T)
    Fv, keep = _device_frame(fa, pv)
    Fp, keep2 = _device_frame(fa)                               # pose fields zero: the posed call must not read them
    pp = N.ProjParams(5.0, 100.0, 0.8, 0.5, 1.5, *criteria)
    d_lms, d_pv, L, ex = dev(lms), dev(np.array([pv])), len(lms), tracker._ex
    outs = []
    for posed in (False, True):
        o = out_buf(L * 4), out_buf(L * 4), out_buf(4)
        if posed:
            tracker.search_by_projection_posed_device(Fp, d_pv.ptr, d_lms.ptr, L, pp, o[0].ptr, o[1].ptr, o[2].ptr)
        else:
            N.check(ex._h, ex._lib.hs_search_by_projection_device(ex._h, C.byref(Fv), d_lms.ptr, L, C.byref(pp), o[0].ptr, o[1].ptr, o[2].ptr, None))
        ex.synchronize()
        outs.append((read(o[0], np.int32, L), read(o[1], np.float32, L), read(o[2], np.int32, 1)))
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    assert outs[0][2][0] > 20


class Chain:
    """one case of track_cases on the device: inputs, state, every output buffer (guarded) and the work area"""

    def __init__(self, tracker, c):
        from hyslam_amd import _native as N
        self.N, self.tr, self.c = N, tracker, c
        fr = c["frame"]
        self.n, self.n_last, self.L, self.cap = len(fr["kps"]), len(c["last_kp_lm"]), len(c["lms"]), c["cap"]
        self.F, self.fkeep = _device_frame(fr)
        order = ("lm_obs_offsets", "lm_obs_kf", "lm_obs_octave", "lm_bad", "lm_nobs", "kf_bad", "kf_id")
        self.tkeep = [dev(c["T"][k]) for k in order]
        self.KT = N.KfTable(self.L, len(c["T"]["kf_id"]), *[b.ptr for b in self.tkeep])
        self.d_lms = dev(np.ascontiguousarray(c["lms"], N.LM_DTYPE))
        self.d_Tpred = dev(np.ascontiguousarray(c["Tcw_pred"], np.float32))
        self.d_last_kps, self.d_last_kp_lm = dev(np.ascontiguousarray(c["last_kps"], N.KP_DTYPE)), dev(c["last_kp_lm"])
        self.d_neigh, self.d_parent = dev(c["neigh"]), dev(c["parent"])
        tp = c["tp"]
        self.tp = N.TrackParams(tp.th_motion, tp.th_motion_wide, tp.n_min_matches, tp.th_local, tp.nnratio_motion, tp.nnratio_local, tp.th_high, tp.sigma_ref,
                                tp.n_max_local_keyframes, tp.n_neighbor_keyframes)
        # a dirty state: the motion model clears it
        rng = np.random.default_rng(5)
        self.state = [guarded(rng.integers(-1, self.L, self.n).astype(np.int32)), guarded(rng.integers(0, 3, self.n).astype(np.uint8)),
                      guarded(np.array([17], np.int32)), guarded(rng.integers(-1, 3, self.n).astype(np.int32))]
        self.ST = N.TrackState(*[b.ptr for b in self.state])
        sizes = dict(n=self.n, n_last=self.n_last, n_kf=self.KT.n_kf, cap=self.cap)
        self.spec = {}

        def alloc(spec, prefix=""):
            ptrs = []
            for k, kind, cnt in spec:
                dt, cnt = N.track_out_dtype(kind), sizes.get(cnt, cnt)
                self.spec[prefix + k] = (out_buf(dt.itemsize * cnt), dt, cnt)
                ptrs.append(self.spec[prefix + k][0].ptr)
            return ptrs
        head, local, tail = alloc(N.TRACK_OUT_HEAD), alloc(N.LOCAL_MAP_OUT_SPEC, "local."), alloc(N.TRACK_OUT_TAIL)
        self.out = N.TrackOut(*head, N.LocalMapOut(*local), *tail)
        self.work_bytes = tracker.track_work_bytes(self.n, self.n_last, self.L, self.cap)
        self.work = out_buf(self.work_bytes)
        self.stream = hipmem.Stream()

    def ptr(self, k, index=0):
        b, dt, _ = self.spec[k]
        return b.ptr + index * dt.itemsize

    def motion(self):
        self.tr.track_motion_model_device(self.F, self.d_Tpred.ptr, self.d_last_kps.ptr, self.d_last_kp_lm.ptr, self.n_last, self.KT, self.d_lms.ptr, self.tp,
                                          self.ST, self.out, self.work.ptr, self.stream.ptr)

    def local(self):
        off = self.N.POSE_RESULT_DTYPE.fields["Tcw"][1]
        self.tr.track_local_map_device(self.F, self.ptr("pose_motion") + off, self.KT, self.d_lms.ptr, self.d_neigh.ptr, 10, self.d_parent.ptr, self.cap, self.tp,
                                       self.ST, self.out, self.work.ptr, self.stream.ptr)

    def frame(self):
        self.tr.track_frame_device(self.F, self.d_Tpred.ptr, self.d_last_kps.ptr, self.d_last_kp_lm.ptr, self.n_last, self.KT, self.d_lms.ptr, self.d_neigh.ptr, 10,
                                   self.d_parent.ptr, self.cap, self.tp, self.ST, self.out, self.work.ptr, self.stream.ptr)

    def results(self):
        self.stream.synchronize()
        read(self.work, np.uint8, self.work_bytes)
        got = {k: read(b, dt, cnt) for k, (b, dt, cnt) in self.spec.items()}
        got["kp_lm"], got["kp_outl"] = read(self.state[0], np.int32, self.n), read(self.state[1], np.uint8, self.n)
        got["n_matches"], got["kp_lm_obs"] = read(self.state[2], np.int32, 1), read(self.state[3], np.int32, self.n)
        return got

    # the same chain from the public device calls, the host doing what k_last_gather, k_track_clear, k_track_select and k_track_gate do
    def parts(self):
        N, tr, ex, c, s, o = self.N, self.tr, self.tr._ex, self.c, self.stream.ptr, self.out
        put = lambda buf, a: hipmem._ok(hipmem.hip().hipMemcpy(buf.ptr, np.ascontiguousarray(a).ctypes.data, a.nbytes, 1), "hipMemcpy H2D")
        Fs = N.FrameView.from_buffer_copy(self.F)
        Fs.kp_lm_obs = self.state[3].ptr
        tp = c["tp"]
        tr.pose_views_device(self.d_Tpred.ptr, self.ptr("pose_view", 0), s)
        prob = np.zeros(1, N.POSE_PROBLEM_DTYPE)
        prob["Tcw"][0] = c["Tcw_pred"].ravel()
        prob["fx"], prob["fy"], prob["cx"], prob["cy"], prob["bf"] = (c["frame"][k] for k in ("fx", "fy", "cx", "cy", "mbf"))
        self.stream.synchronize()
        hipmem._ok(hipmem.hip().hipMemcpy(self.ptr("problem", 0), prob.ctypes.data, prob.nbytes, 1), "hipMemcpy H2D")
        put(self.spec["last_lms"][0], np.ascontiguousarray(R.gather_last(c["lms"], c["last_kp_lm"], c["last_kps"]), N.LM_DTYPE))
        for buf, a in zip(self.state, (np.full(self.n, -1, np.int32), np.zeros(self.n, np.uint8), np.zeros(1, np.int32), np.full(self.n, -1, np.int32))):
            put(buf, a)
        for name, th in (("narrow", tp.th_motion), ("wide", tp.th_motion_wide)):
            pp = N.ProjParams(th, tp.th_high, tp.nnratio_motion, 0.5, 1.5, 0, 1, 1, sigma_ref=tp.sigma_ref)
            tr.search_by_projection_posed_device(Fs, self.ptr("pose_view", 0), self.ptr("last_lms"), self.n_last, pp, self.ptr(name + "_idx"),
                                                 self.ptr(name + "_dist"), self.ptr(name + "_n"), s)
        self.stream.synchronize()
        nn, nw = (int(read(self.spec[k][0], np.int32, 1)[0]) for k in ("narrow_n", "wide_n"))
        wide = nn < tp.n_min_matches
        failed = (nw if wide else nn) < tp.n_min_matches
        put(self.spec["op_view"][0], read(self.spec["wide_idx" if wide else "narrow_idx"][0], np.int32, self.n_last))
        res = np.zeros(1, N.TRACK_RESULT_DTYPE)
        res["status"], res["used_wide"], res["n_narrow"], res["n_wide"] = int(failed), int(wide), nn, nw
        put(self.spec["result"][0], res)
        tr.frame_associate_device(self.n, self.L, self.state[0].ptr, self.state[1].ptr, self.state[2].ptr, self.n_last, self.ptr("op_view"), self.d_last_kp_lm.ptr,
                                  self.work.ptr, s)
        ex.pose_edges_device(Fs, self.d_lms.ptr, self.L, self.state[0].ptr, self.ptr("edges_motion"), self.n, self.ptr("n_edges_motion", 0), tp.sigma_ref, None, s)
        self.stream.synchronize()
        ne = read(self.spec["n_edges_motion"][0], np.int32, 2)
        ne[1] = 0 if failed else ne[0]
        put(self.spec["n_edges_motion"][0], ne)
        ex.pose_optimize_device(1, self.ptr("problem", 0), self.ptr("edges_motion"), self.ptr("outlier_motion"), self.ptr("pose_motion"), None,
                                self.ptr("n_edges_motion", 1), self.n, None, s)
        off_map = N.TRACK_RESULT_DTYPE.fields["n_matches_map"][1]
        tr.track_discard_device(N.HS_TRACK_MOTION, self.ptr("edges_motion"), self.ptr("n_edges_motion", 1), self.n, self.ptr("outlier_motion"), self.ptr("pose_motion"),
                                self.KT, c["frame"]["sensor"], self.state[0].ptr, self.state[1].ptr, self.state[2].ptr, self.ptr("result") + off_map, s)
        # ---- TrackLocalMap
        d_Tin = self.ptr("pose_motion") + N.POSE_RESULT_DTYPE.fields["Tcw"][1]
        tr.pose_views_device(d_Tin, self.ptr("pose_view", 1), s)
        self.stream.synchronize()
        prob["Tcw"][0] = read(self.spec["pose_motion"][0], N.POSE_RESULT_DTYPE, 1)["Tcw"][0]
        hipmem._ok(hipmem.hip().hipMemcpy(self.ptr("problem", 1), prob.ctypes.data, prob.nbytes, 1), "hipMemcpy H2D")
        tr.frame_views_device(self.n, self.state[0].ptr, self.state[1].ptr, self.state[2].ptr, self.KT, 1, self.state[3].ptr, s)
        pp = N.ProjParams(tp.th_local, tp.th_high, tp.nnratio_local, 0.5, 1.5, 1, 1, 0, sigma_ref=tp.sigma_ref)
        assoc_bytes = tr.track_work_bytes(self.n, 0, self.L, 0) - ex.local_map_work_bytes(self.L)       # the local map's work area follows the replay's
        lm_work = out_buf(ex.local_map_work_bytes(self.L))
        tr.local_map_search_posed_device(self.KT, self.state[0].ptr, self.n, self.d_neigh.ptr, 10, self.d_parent.ptr, tp.n_max_local_keyframes,
                                         tp.n_neighbor_keyframes, Fs, self.ptr("pose_view", 1), self.d_lms.ptr, pp, self.cap, o.local, lm_work.ptr, s)
        tr.frame_associate_device(self.n, self.L, self.state[0].ptr, self.state[1].ptr, self.state[2].ptr, self.cap, o.local.match_idx, o.local.sel, self.work.ptr, s)
        ex.pose_edges_device(Fs, self.d_lms.ptr, self.L, self.state[0].ptr, self.ptr("edges_local"), self.n, self.ptr("n_edges_local"), tp.sigma_ref, None, s)
        ex.pose_optimize_device(1, self.ptr("problem", 1), self.ptr("edges_local"), self.ptr("outlier_local"), self.ptr("pose_local"), None, self.ptr("n_edges_local"),
                                self.n, None, s)
        tr.track_discard_device(N.HS_TRACK_LOCAL, self.ptr("edges_local"), self.ptr("n_edges_local"), self.n, self.ptr("outlier_local"), self.ptr("pose_local"),
                                self.KT, c["frame"]["sensor"], self.state[0].ptr, self.state[1].ptr, self.state[2].ptr,
                                self.ptr("result") + N.TRACK_RESULT_DTYPE.fields["n_inliers"][1], s)
        self.stream.synchronize()
        read(lm_work, np.uint8, ex.local_map_work_bytes(self.L))
        assert assoc_bytes > 0


@pytest.mark.parametrize("name", ["narrow", "wide", "both_fail", "too_few_edges"])
def test_frame_call_is_its_parts(tracker, name):
    c, _ = TC.directed(name)
    fused, staged, apart = Chain(tracker, c), Chain(tracker, c), Chain(tracker, c)
    fused.frame()
    staged.motion(); staged.local()
    apart.parts()
    f, s, a = fused.results(), staged.results(), apart.results()
    same_outputs(f, s, "two stage calls")
    same_outputs(f, a, "public calls one by one")


def test_posed_local_map_equals_the_call_by_value(tracker):
    """the local map's search with the pose in the launch arguments against the posed sibling, on the state the motion stage leaves"""
    from hyslam_amd import _native as N
    c, (m, _) = TC.directed("narrow")
    outs = []
    for posed in (False, True):
        ch = Chain(tracker, c)
        pv = R.pose_view(m["pose"]["Tcw"])
        kp_lm, obs = m["state"][0], R.lm_obs_of(R.DenseMatches.from_dense(*m["state"]), ch.n, c["T"]["lm_nobs"])
        d_flm, d_obs, d_pv = dev(kp_lm), dev(obs), dev(np.array([pv]))
        F, keep = _device_frame(c["frame"], None if posed else pv)
        F.kp_lm_obs = d_obs.ptr
        pp = N.ProjParams(3.0, 100.0, 0.8, 0.5, 1.5, 1, 1, 0)
        lm_work = out_buf(tracker._ex.local_map_work_bytes(ch.L))
        if posed:
            tracker.local_map_search_posed_device(ch.KT, d_flm.ptr, ch.n, ch.d_neigh.ptr, 10, ch.d_parent.ptr, 80, 10, F, d_pv.ptr, ch.d_lms.ptr, pp, ch.cap,
                                                  ch.out.local, lm_work.ptr, ch.stream.ptr)
        else:
            tracker._ex.local_map_search_device(ch.KT, d_flm.ptr, ch.n, ch.d_neigh.ptr, 10, ch.d_parent.ptr, 80, 10, F, ch.d_lms.ptr, pp, ch.cap, ch.out.local,
                                                lm_work.ptr, ch.stream.ptr)
        ch.stream.synchronize()
        outs.append({k: read(b, dt, cnt) for k, (b, dt, cnt) in ch.spec.items() if k.startswith("local.")})
    for k in outs[0]:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
    assert outs[0]["local.n_matches"][0] > 20


# ---------------------------------------------------------------- discard and frame views against numpy
def _discard_numpy(mode, sensor, edges_kp, ne, outlier, ran, kp_lm, kp_outl, nm, lm_nobs):
    kp_lm, kp_outl, count = kp_lm.copy(), kp_outl.copy(), 0
    for k in range(ne):
        i = edges_kp[k]
        if ran and kp_outl[i]:                                  # setOutlier: nothing without an `outliers` entry
            kp_outl[i] = 2 if outlier[k] else 1
        if kp_lm[i] < 0:                                        # the loop walks the associations
            continue
        if kp_outl[i] == 2:
            if mode == 0 or sensor == 1:
                kp_lm[i], kp_outl[i], nm = -1, 0, nm - 1
        elif lm_nobs[kp_lm[i]] > 0:
            count += 1
    return kp_lm, kp_outl, nm, count


def discard_device(tracker, mode, sensor, edges_kp, n_edges, edge_cap, outlier, status, kp_lm, kp_outl, nm, lm_nobs, stream=None):
    """hs_track_discard_device on guarded copies -> (kp_lm, kp_outl, n_matches, count); n_edges: the value of *d_n_edges (may exceed edge_cap)"""
    from hyslam_amd import _native as N
    n, L = len(kp_lm), len(lm_nobs)
    edges = np.zeros(len(edges_kp), N.POSE_EDGE_DTYPE)
    edges["kp"] = edges_kp
    result = np.zeros(1, N.POSE_RESULT_DTYPE)
    result["status"] = status
    d_nobs = dev(lm_nobs)
    KT = N.KfTable(L, 0, None, None, None, None, d_nobs.ptr, None, None)
    d_lm, d_outl, d_nm, d_cnt = guarded(kp_lm), guarded(kp_outl), guarded(np.array([nm], np.int32)), out_buf(4)
    ins = dev(edges), dev(np.array([n_edges], np.int32)), dev(outlier), dev(result)
    st = stream or hipmem.Stream()
    tracker.track_discard_device(mode, ins[0].ptr, ins[1].ptr, edge_cap, ins[2].ptr, ins[3].ptr, KT, sensor, d_lm.ptr, d_outl.ptr, d_nm.ptr, d_cnt.ptr, st.ptr)
    st.synchronize()
    return read(d_lm, np.int32, n), read(d_outl, np.uint8, n), int(read(d_nm, np.int32, 1)[0]), int(read(d_cnt, np.int32, 1)[0])


@pytest.mark.parametrize("mode,sensor,status,truncate", [(0, 1, 0, False), (0, 0, 0, True), (1, 1, 0, False), (1, 0, 0, False), (1, 2, 2, True), (0, 1, 1, False),
                                                         (1, 1, 1, False)])
def test_discard_against_numpy(tracker, mode, sensor, status, truncate):
    n, L = 1500, 700
    rng = np.random.default_rng(100 * mode + 10 * sensor + status)
    kp_lm = np.where(rng.random(n) < 0.7, rng.integers(0, L, n), -1).astype(np.int32)
    kp_outl = rng.integers(0, 3, n).astype(np.uint8)            # also what the chain never makes: a held view without an entry, a flagged empty view
    lm_nobs = rng.integers(0, 3, L).astype(np.int32)
    with_edge = (kp_lm >= 0) | (rng.random(n) < 0.1)            # ... and an edge on a view that holds nothing
    edges_kp = np.nonzero(with_edge)[0]
    outlier = (rng.random(len(edges_kp)) < 0.3).astype(np.uint8)
    cap = len(edges_kp) // 2 if truncate else len(edges_kp)
    want = _discard_numpy(mode, sensor, edges_kp, min(len(edges_kp), cap), outlier, status != 1, kp_lm, kp_outl, 900, lm_nobs)
    got = discard_device(tracker, mode, sensor, edges_kp, len(edges_kp), cap, outlier, status, kp_lm, kp_outl, 900, lm_nobs)
    for w, g, what in zip(want, got, ("kp_lm", "kp_outl", "n_matches", "count")):
        assert np.array_equal(w, g), what
    if status == 1:
        stays = got[0] == kp_lm                                 # TOO_FEW: no flag is set from `outlier`; a view flagged BEFORE the call is still discarded
        assert np.array_equal(got[1][stays], kp_outl[stays]) and ((kp_outl[~stays] == 2) & (got[1][~stays] == 0)).all()
        assert (~stays).any() == (mode == 0 or sensor == 1)


def _frame_views_numpy(kp_lm, kp_outl, nm, lm_bad, lm_nobs, drop_bad):
    """-> (kp_lm, kp_outl, n_matches, kp_lm_obs)"""
    bad = (kp_lm >= 0) & (lm_bad[np.maximum(kp_lm, 0)] != 0) & bool(drop_bad)
    want_lm = np.where(bad, -1, kp_lm)
    want_outl = np.where(bad, 0, kp_outl)
    want_obs = np.where(want_lm >= 0, lm_nobs[np.maximum(want_lm, 0)], -1)
    return want_lm, want_outl, nm - int(bad.sum()), want_obs


def frame_views_device(tracker, kp_lm, kp_outl, nm, lm_bad, lm_nobs, drop_bad, stream=None):
    from hyslam_amd import _native as N
    n, L = len(kp_lm), len(lm_nobs)
    tabs = dev(lm_bad), dev(lm_nobs)
    KT = N.KfTable(L, 0, None, None, None, tabs[0].ptr, tabs[1].ptr, None, None)
    d_lm, d_outl, d_nm, d_obs = guarded(kp_lm), guarded(kp_outl), guarded(np.array([nm], np.int32)), out_buf(n * 4)
    st = stream or hipmem.Stream()
    tracker.frame_views_device(n, d_lm.ptr, d_outl.ptr, d_nm.ptr, KT, drop_bad, d_obs.ptr, st.ptr)
    st.synchronize()
    return read(d_lm, np.int32, n), read(d_outl, np.uint8, n), int(read(d_nm, np.int32, 1)[0]), read(d_obs, np.int32, n)


@pytest.mark.parametrize("drop_bad", [0, 1])
@pytest.mark.parametrize("n", [1, 1023, 1025, 3000])
def test_frame_views_against_numpy(tracker, n, drop_bad):
    L = 500
    rng = np.random.default_rng(n + drop_bad)
    kp_lm = np.where(rng.random(n) < 0.7, rng.integers(0, L, n), -1).astype(np.int32)
    kp_outl = rng.integers(0, 3, n).astype(np.uint8)
    lm_nobs, lm_bad = rng.integers(0, 5, L).astype(np.int32), (rng.random(L) < 0.2).astype(np.uint8)
    want = _frame_views_numpy(kp_lm, kp_outl, n, lm_bad, lm_nobs, drop_bad)
    got = frame_views_device(tracker, kp_lm, kp_outl, n, lm_bad, lm_nobs, drop_bad)
    for w, g, what in zip(want, got, ("kp_lm", "kp_outl", "n_matches", "kp_lm_obs")):
        assert np.array_equal(w, g), what


# ---------------------------------------------------------------- end to end against the reference
def check_case(tracker, c, ref, report):
    ch = Chain(tracker, c)
    ch.frame()
    got = ch.results()
    return compare_track(got, c, ref, report, ch.N.LM_DTYPE)


@pytest.mark.parametrize("name", list(TC.DIRECTED))
def test_end_to_end_directed(tracker, name):
    c, ref = TC.directed(name)
    check_case(tracker, c, ref, name)


def test_end_to_end_random(tracker):
    cases, drawn = TC.random_cases()
    assert len(cases) == TC.N_RANDOM
    for c, ref in cases:
        check_case(tracker, c, ref, "seed %d" % c["seed"])


def test_refusals(tracker):
    """what only a LATER stage of a chain reads — the frame's uR under a stereo sensor, the local map's outputs, neigh, parent, two of its tables, cap —
    is refused by hs_track_motion_model_device / _local_map_ / _frame_ on the host, before the first launch: each gives HS_ERR_INVALID and every output
    byte, the work area and the state keep their bytes (n = 300, stereo); the valid call then reproduces the reference"""
    from hyslam_amd import _native as N
    c, ref = TC.directed("narrow")
    assert c["frame"]["sensor"] != 0 and len(c["frame"]["kps"]) == 300
    ch = Chain(tracker, c)
    lib, h = tracker._ex._lib, tracker._ex._h
    state_bytes = [b.to_numpy(np.uint8, nb + GUARD).copy() for b, nb in zip(ch.state, (4 * ch.n, ch.n, 4, 4 * ch.n))]
    d_Tin = ch.ptr("pose_motion") + N.POSE_RESULT_DTYPE.fields["Tcw"][1]

    def args(**kw):
        a = dict(F=ch.F, T=ch.KT, out=ch.out, neigh=ch.d_neigh.ptr, neigh_cap=10, parent=ch.d_parent.ptr, cap=ch.cap)
        a.update(kw)
        return a

    def motion(**kw):
        a = args(**kw)
        return lib.hs_track_motion_model_device(h, C.byref(a["F"]), ch.d_Tpred.ptr, ch.d_last_kps.ptr, ch.d_last_kp_lm.ptr, ch.n_last, C.byref(a["T"]), ch.d_lms.ptr,
                                                C.byref(ch.tp), C.byref(ch.ST), C.byref(a["out"]), ch.work.ptr, ch.stream.ptr)

    def local(**kw):
        a = args(**kw)
        return lib.hs_track_local_map_device(h, C.byref(a["F"]), d_Tin, C.byref(a["T"]), ch.d_lms.ptr, a["neigh"], a["neigh_cap"], a["parent"], a["cap"], C.byref(ch.tp),
                                             C.byref(ch.ST), C.byref(a["out"]), ch.work.ptr, ch.stream.ptr)

    def frame(**kw):
        a = args(**kw)
        return lib.hs_track_frame_device(h, C.byref(a["F"]), ch.d_Tpred.ptr, ch.d_last_kps.ptr, ch.d_last_kp_lm.ptr, ch.n_last, C.byref(a["T"]), ch.d_lms.ptr, a["neigh"],
                                         a["neigh_cap"], a["parent"], a["cap"], C.byref(ch.tp), C.byref(ch.ST), C.byref(a["out"]), ch.work.ptr, ch.stream.ptr)

    def without(struct, field, value=None):
        s = type(struct).from_buffer_copy(struct)
        setattr(s, field, value)
        return s

    def out_without(field):
        o = type(ch.out).from_buffer_copy(ch.out)
        setattr(o.local, field, None)
        return o
    no_uR = dict(F=without(ch.F, "uR"))
    later = [no_uR, dict(out=out_without("weights")), dict(out=out_without("match_idx")), dict(parent=None), dict(neigh=None),
             dict(T=without(ch.KT, "lm_obs_offsets")), dict(T=without(ch.KT, "kf_bad"))]
    assert motion(**no_uR) == N.HS_ERR_INVALID
    for kw in later:
        for f in (local, frame):
            assert f(**kw) == N.HS_ERR_INVALID, (f.__name__, list(kw))
    assert frame(cap=0) == N.HS_ERR_INVALID and local(cap=0) == N.HS_ERR_INVALID and frame(neigh_cap=-1) == N.HS_ERR_INVALID
    tracker._ex.synchronize()
    ch.stream.synchronize()
    for k, (b, dt, cnt) in ch.spec.items():
        assert (b.to_numpy(np.uint8, dt.itemsize * cnt + GUARD) == 0x55).all(), (k, "an output of a refused call was written")
    assert (ch.work.to_numpy(np.uint8, ch.work_bytes + GUARD) == 0x55).all(), "the work area of a refused call was written"
    for b, was, k in zip(ch.state, state_bytes, ("kp_lm", "kp_outl", "n_matches", "kp_lm_obs")):
        assert np.array_equal(b.to_numpy(np.uint8, len(was)), was), (k, "the state was touched by a refused call")
    # the handle is as good as before
    ch.frame()
    compare_track(ch.results(), c, ref, "after the refusals", ch.N.LM_DTYPE)


def test_frame_tracker_returns_what_the_device_calls_compute(tracker):
    from hyslam_amd import _native as N
    c, ref = TC.directed("outlier_removed")
    got = check_case(tracker, c, ref, "outlier_removed")
    tp = c["tp"]
    prm = N.TrackParams(tp.th_motion, tp.th_motion_wide, tp.n_min_matches, tp.th_local, tp.nnratio_motion, tp.nnratio_local, tp.th_high, tp.sigma_ref,
                        tp.n_max_local_keyframes, tp.n_neighbor_keyframes)
    res = tracker.TrackFrame(c["frame"], c["Tcw_pred"], c["last_kps"], c["last_kp_lm"], c["T"], c["lms"], c["neigh"], c["parent"], params=prm, cap=c["cap"])
    assert np.array_equal(res["kp_lm"], got["kp_lm"]) and np.array_equal(res["kp_outl"], got["kp_outl"]) and res["n_matches"] == int(got["n_matches"][0])
    assert res["pose_motion"].tobytes() == got["pose_motion"][0].tobytes() and res["pose_local"].tobytes() == got["pose_local"][0].tobytes()
    r = got["result"][0]
    assert (res["status"], res["used_wide"], res["n_narrow"], res["n_wide"], res["n_matches_map"], res["n_inliers"]) == \
        (int(r["status"]), bool(r["used_wide"]), int(r["n_narrow"]), int(r["n_wide"]), int(r["n_matches_map"]), int(r["n_inliers"]))
    # the two stages through their own methods give the same state
    m = tracker.TrackMotionModel(c["frame"], c["Tcw_pred"], c["last_kps"], c["last_kp_lm"], c["T"], c["lms"], params=prm)
    l = tracker.TrackLocalMap(c["frame"], m["pose_motion"]["Tcw"], c["T"], c["lms"], c["neigh"], c["parent"], m["kp_lm"], m["kp_outl"], m["n_matches"], params=prm,
                              cap=c["cap"])
    assert np.array_equal(l["kp_lm"], res["kp_lm"]) and np.array_equal(l["kp_outl"], res["kp_outl"]) and l["n_inliers"] == res["n_inliers"]
