"""GPU: the local map between the key-frame vote and the projection search — hs_local_keyframes(_device), hs_local_points(_device),
hs_landmark_gather_device and hs_local_map_search_device — against the restatement in tests/ref_localmap.py (pinned by tests/test_localmap_ref.py).
Integer and index results: EVERY output is compared exactly.  Through the C ABI, the Python methods and the device forms on a caller stream with
sentinel-filled outputs and guard bytes; the gather byte for byte; the fused call against its five separate calls and against ref_localmap + the
numpy projection search on a 640 x 480 scene."""
import ctypes as C

import numpy as np
import pytest

import hipmem
import ref_kfgraph as RK
import ref_localmap as R
from kfgraph_cases import key_frame_queries, random_table
from localmap_cases import KNOWN_KEYFRAMES, KNOWN_POINTS, POINTS_TABLE, random_keyframes, random_points

pytestmark = pytest.mark.gpu

GUARD = 64            # bytes behind every device output, filled with 0x55 and checked


@pytest.fixture(scope="module")
def matcher(gpu):
    import hyslam_amd as HS
    return HS.FeatureMatcher(extractor=HS.ORBExtractor(device=0))


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def dev(a):
    return hipmem.DevBuf.from_numpy(np.ascontiguousarray(a))


def out_buf(nbytes):
    b = hipmem.DevBuf(nbytes + GUARD)
    b.fill(0x55)
    return b


def read(buf, dtype, count):
    """`count` elements, after checking that the guard behind them is untouched"""
    nbytes = np.dtype(dtype).itemsize * count
    raw = buf.to_numpy(np.uint8, nbytes + GUARD)
    assert (raw[nbytes:] == 0x55).all(), "bytes written behind the output"
    return raw[:nbytes].view(dtype).copy()


def native_table(T, on_device=False):
    from hyslam_amd import _native as N
    order = ("lm_obs_offsets", "lm_obs_kf", "lm_obs_octave", "lm_bad", "lm_nobs", "kf_bad", "kf_id")
    if on_device:
        keep = [dev(T[k]) for k in order]
        return N.KfTable(len(T["lm_bad"]), len(T["kf_id"]), *[b.ptr for b in keep]), keep
    keep = [np.ascontiguousarray(T[k]) for k in order]
    return N.KfTable(len(T["lm_bad"]), len(T["kf_id"]), *[a.ctypes.data for a in keep]), keep


def keyframes_device(ex, c, stream):
    n_kf = len(c["weights"])
    ins = [dev(c[k]) for k in ("weights", "kf_bad", "neigh", "parent")]
    d_local, d_n = out_buf(n_kf), out_buf(4)
    ex.local_keyframes_device(n_kf, ins[0].ptr, ins[1].ptr, ins[2].ptr, c["neigh"].shape[1], ins[3].ptr, c["n_max"], c["n_neighbor"], d_local.ptr, d_n.ptr,
                              stream.ptr)
    stream.synchronize()
    return read(d_local, np.uint8, n_kf), int(read(d_n, np.int32, 1)[0])


def points_device(ex, T, local, flm, cap, stream):
    KT, keep = native_table(T, on_device=True)
    d_local, d_flm = dev(local), dev(flm)
    d_rem, d_sel, d_n = out_buf(len(flm)), out_buf(cap * 4), out_buf(4)
    work = out_buf(ex.local_points_work_bytes(KT.L))
    ex.local_points_device(KT, d_local.ptr, d_flm.ptr, len(flm), d_rem.ptr, d_sel.ptr, cap, d_n.ptr, work.ptr, stream.ptr)
    stream.synchronize()
    read(work, np.uint8, ex.local_points_work_bytes(KT.L))
    return dict(frame_remove=read(d_rem, np.uint8, len(flm)), sel=read(d_sel, np.int32, cap), n_sel=int(read(d_n, np.int32, 1)[0]))


# ---- known answers
@pytest.mark.parametrize("name", sorted(KNOWN_KEYFRAMES))
def test_known_keyframes(matcher, name):
    c = KNOWN_KEYFRAMES[name]
    local, n_local = matcher.LocalKeyFrames(c["weights"], c["kf_bad"], c["neigh"], c["parent"], c["n_max"], c["n_neighbor"])
    assert np.nonzero(local)[0].tolist() == c["local"] and n_local == len(c["local"]) and local.max(initial=0) <= 1, (name, local)
    local, n_local = keyframes_device(matcher._ex, c, hipmem.Stream())
    assert np.nonzero(local)[0].tolist() == c["local"] and n_local == len(c["local"]) and local.max(initial=0) <= 1, (name, "device", local)


@pytest.mark.parametrize("name", sorted(KNOWN_POINTS))
def test_known_points(matcher, name):
    c = KNOWN_POINTS[name]
    rem, sel, n_sel = matcher.LocalPoints(POINTS_TABLE, c["local"], c["frame_lm"], cap=c["cap"])
    got_d = points_device(matcher._ex, POINTS_TABLE, c["local"], c["frame_lm"], c["cap"], hipmem.Stream())
    for got in (dict(frame_remove=rem, sel=sel, n_sel=n_sel), got_d):
        for k in R.POINT_KEYS:
            assert np.array_equal(got[k], np.asarray(c[k])), (name, k, got[k])


# ---- random cases on the sizes where the kernels change their path
@pytest.mark.parametrize("n_kf", [1, 63, 64, 65, 129])
def test_keyframes_sizes(matcher, n_kf):
    """one 64-slot word less one, exactly one, one more, two and one; every way the walk can end (tests/test_localmap_ref.py counts them)"""
    s = hipmem.Stream()
    grew = 0
    for seed in range(12):
        c = random_keyframes(1000 * n_kf + seed, n_kf, neigh_cap=int(np.random.default_rng(seed).choice([1, 10, 70])))
        want, n_want = R.local_keyframes_fast(c["weights"], c["kf_bad"], c["neigh"], c["parent"], c["n_max"], c["n_neighbor"])
        local, n_local = matcher.LocalKeyFrames(c["weights"], c["kf_bad"], c["neigh"], c["parent"], c["n_max"], c["n_neighbor"])
        assert np.array_equal(local, want) and n_local == n_want, (n_kf, seed, "host form")
        local, n_local = keyframes_device(matcher._ex, c, s)
        assert np.array_equal(local, want) and n_local == n_want, (n_kf, seed, "device form")
        grew += n_want > int(((c["weights"] > 0) & (c["kf_bad"] == 0)).sum())
    assert grew > 0 or n_kf == 1


def test_keyframes_long_walk(matcher):
    """no parents, no limit: every member is visited and each brings its neighbour in — a chain that runs through all of 129 slots"""
    n_kf = 129
    ng = np.full((n_kf, 2), -1, np.int32)
    ng[:-1, 0] = np.arange(1, n_kf)
    c = dict(weights=np.eye(1, n_kf, 0, dtype=np.int32)[0], kf_bad=np.zeros(n_kf, np.uint8), neigh=ng, parent=np.full(n_kf, -1, np.int32), n_max=-1, n_neighbor=2)
    for local, n_local in (matcher.LocalKeyFrames(c["weights"], c["kf_bad"], ng, c["parent"], -1, 2), keyframes_device(matcher._ex, c, hipmem.Stream())):
        assert n_local == n_kf and local.all()
    c["n_max"] = 40                                                                       # stops at the member visited with 41 in the set
    local, n_local = keyframes_device(matcher._ex, c, hipmem.Stream())
    assert n_local == 41 and local[:41].all() and not local[41:].any()


def _block():
    from hyslam_amd import _native as N
    return N.HS_LOCAL_POINTS_BLOCK


@pytest.mark.parametrize("which", ["0", "1", "block-1", "block", "block+1", "3*block+1"])
def test_points_sizes(matcher, which):
    """L around the compaction block; observation lists from 0 to 300 entries; cap below, at and above n_sel"""
    B = _block()
    L = {"0": 0, "1": 1, "block-1": B - 1, "block": B, "block+1": B + 1, "3*block+1": 3 * B + 1}[which]
    n_kf = 400 if L > B else 65
    big = [(3, 300), (B - 1, 150), (B, 200)] if L > B else ([(0, 65)] if L else [])
    T, local, flm = random_points(L + 5, n_kf, L, max_obs=12, big=big, n_assoc=300 if L else 7, p_local=0.15)
    if L == 1:
        T["lm_bad"][0], flm[:] = 0, -1                                                    # the one landmark is selected
    full = R.local_points_fast(T, local, flm, L)
    n = full["n_sel"]
    assert L < B or (n > B // 4 and full["frame_remove"].any())
    s = hipmem.Stream()
    for cap in sorted({0, max(n - 1, 0), n, n + 3, L}):
        want = R.local_points_fast(T, local, flm, cap)
        rem, sel, n_sel = matcher.LocalPoints(T, local, flm, cap=cap)
        assert R.same(dict(frame_remove=rem, sel=sel, n_sel=n_sel), want) is None, (which, cap, "host form")
        assert R.same(points_device(matcher._ex, T, local, flm, cap, s), want) is None, (which, cap, "device form")
    # the same call twice gives the same list: no position depends on the order in which blocks or atomics arrive
    a, b = points_device(matcher._ex, T, local, flm, L, s), points_device(matcher._ex, T, local, flm, L, s)
    assert np.array_equal(a["sel"], b["sel"])


def test_points_device_skips_slots_outside_the_table(matcher):
    """the device form checks nothing: an observation by a slot outside [0, n_kf) and an association outside [0, L) are skipped"""
    T, local, flm = random_points(77, 30, 500, n_assoc=50, p_local=0.4)
    T["lm_obs_kf"] = T["lm_obs_kf"].copy()
    T["lm_obs_kf"][::7] = 30
    T["lm_obs_kf"][3::11] = -2
    flm[5], flm[6] = 500, -9
    want = R.local_points_fast(T, local, flm, 500)
    assert want["n_sel"] > 50
    assert R.same(points_device(matcher._ex, T, local, flm, 500, hipmem.Stream()), want) is None


def test_host_forms_refuse_bad_arguments_and_leave_outputs_alone(matcher):
    from hyslam_amd import _native as N
    ex = matcher._ex
    c = random_keyframes(5, 40, neigh_cap=4)
    local, n_local = np.full(40, 99, np.uint8), np.full(1, 99, np.int32)

    def kf(neigh, parent, n_neighbor):
        return ex._lib.hs_local_keyframes(ex._h, 40, p(c["weights"]), p(c["kf_bad"]), p(neigh), 4, p(parent), 80, n_neighbor, p(local), p(n_local))
    bad_neigh, bad_parent = c["neigh"].copy(), c["parent"].copy()
    bad_neigh[7, 1], bad_parent[3] = 40, -2
    for args in ((c["neigh"], c["parent"], 5), (c["neigh"], c["parent"], -1), (bad_neigh, c["parent"], 4), (c["neigh"], bad_parent, 4)):
        assert kf(*args) == N.HS_ERR_INVALID and (local == 99).all() and n_local[0] == 99
    assert kf(c["neigh"], c["parent"], 4) == N.HS_OK and n_local[0] != 99
    T, loc, flm = random_points(6, 20, 300, n_assoc=30)
    rem, sel, n_sel = np.full(30, 99, np.uint8), np.full(300, 99, np.int32), np.full(1, 99, np.int32)

    def pts(T, flm):
        KT, keep = native_table(T)
        return ex._lib.hs_local_points(ex._h, C.byref(KT), p(loc), p(flm), 30, p(rem), p(sel), 300, p(n_sel))
    T2 = dict(T); T2["lm_obs_offsets"] = T["lm_obs_offsets"].copy(); T2["lm_obs_offsets"][100] = T2["lm_obs_offsets"][101] + 2
    T3 = dict(T); T3["lm_obs_kf"] = T["lm_obs_kf"].copy(); T3["lm_obs_kf"][4] = 20
    bad_flm = flm.copy(); bad_flm[2] = 300
    for args in ((T2, flm), (T3, flm), (T, bad_flm)):
        assert pts(*args) == N.HS_ERR_INVALID and (rem == 99).all() and (sel == 99).all() and n_sel[0] == 99
    assert pts(T, flm) == N.HS_OK and n_sel[0] != 99


# ---- the gather
@pytest.mark.parametrize("n_sel,cap", [(0, 5), (37, 37), (37, 64), (64, 37), (200, 333)])
def test_gather_byte_for_byte(matcher, n_sel, cap):
    """against numpy indexing: the records, assoc_kp = -1 / skip = 0 on them, the skip = 1 tail up to cap, and no byte behind cap records"""
    from hyslam_amd import _native as N
    rng = np.random.default_rng(n_sel * 1000 + cap)
    L = 401
    lms = np.frombuffer(rng.integers(0, 256, L * N.LM_DTYPE.itemsize, dtype=np.uint8).tobytes(), N.LM_DTYPE).copy()
    sel = np.full(max(cap, n_sel), -1, np.int32)
    sel[:n_sel] = np.sort(rng.choice(L, n_sel, replace=False))
    sel = sel[:cap]                                                                       # hs_local_points writes only the first cap
    d_lms, d_sel, d_n = dev(lms), dev(sel), dev(np.array([n_sel], np.int32))
    d_out = out_buf(cap * 80)
    s = hipmem.Stream()
    matcher._ex.landmark_gather_device(d_lms.ptr, L, d_sel.ptr, d_n.ptr, cap, d_out.ptr, s.ptr)
    s.synchronize()
    got = read(d_out, np.uint8, cap * 80)
    assert got.tobytes() == R.gather(lms, sel, n_sel, cap).tobytes()
    assert d_lms.to_numpy(np.uint8, L * 80).tobytes() == lms.tobytes()


def test_gather_treats_an_index_outside_the_array_as_empty(matcher):
    from hyslam_amd import _native as N
    lms = np.frombuffer(np.random.default_rng(1).integers(0, 256, 10 * 80, dtype=np.uint8).tobytes(), N.LM_DTYPE).copy()
    sel = np.array([2, 10, -1, 9], np.int32)
    d_out = out_buf(4 * 80)
    bufs = dev(lms), dev(sel), dev(np.array([4], np.int32))
    matcher._ex.landmark_gather_device(bufs[0].ptr, 10, bufs[1].ptr, bufs[2].ptr, 4, d_out.ptr)
    matcher._ex.synchronize()
    got = read(d_out, N.LM_DTYPE, 4)
    want = R.gather(lms, np.array([2, 0, 0, 9], np.int32), 4, 4)
    want[1:3] = np.zeros(2, N.LM_DTYPE)
    want["assoc_kp"][1:3], want["skip"][1:3] = -1, 1
    assert got.tobytes() == want.tobytes()


# ---- the whole chain
@pytest.fixture(scope="module")
def scene():
    """a 640 x 480 stereo frame with a few hundred landmarks around it, a map of 65 key frames that observe them, a frame that holds some of them
    already (null, bad and good ones), and the reference's answer to every stage — computed once"""
    import scenes
    from hyslam_amd import _native as N
    sc = scenes.projection_scene(71, 640, 480, nfeat=200, copies=3)
    lms = np.ascontiguousarray(sc["lms"], N.LM_DTYPE)
    L, n_kf = len(lms), 65
    rng = np.random.default_rng(71)
    T = random_table(71, n_kf, L, max_obs=6, window=True, p_bad_lm=0.08, p_bad_kf=0.1)
    off, q_lm, ids = key_frame_queries(T)
    neigh = RK.votes_fast(T, off, q_lm, ids, 0, 3, 10)["ordered_slot"].copy()            # each slot's getBestCovisibilityKeyFrames(pKF, 10)
    parent = np.full(n_kf, -1, np.int32)
    # the frame holds 60 entries (null, bad and good ones) among the landmarks seen from slots 20 .. 31 only
    lo, hi = T["lm_obs_offsets"][:-1], T["lm_obs_offsets"][1:]
    near = np.nonzero((hi > lo) & (T["lm_obs_kf"][np.minimum(lo, len(T["lm_obs_kf"]) - 1)] >= 20) & (T["lm_obs_kf"][hi - 1] < 32))[0]
    flm = rng.choice(near, 60, replace=False).astype(np.int32)
    flm[::9] = -1
    held = flm[flm >= 0]
    w = RK.votes_fast(T, np.array([0, len(held)], np.int64), held, None, 1, 1, 0)
    members = np.nonzero((w["weights"][0] > 0) & (T["kf_bad"] == 0))[0]
    good = np.nonzero(T["kf_bad"] == 0)[0]
    neigh[members[0], 0] = good[good >= 45][0]                                            # the first member brings a far key frame in ...
    parent[members[3]] = good[good >= 58][0]                                              # ... and the walk ends on the fourth member's parent
    want = dict(weights=w["weights"][0], max_slot=w["max_slot"][0], max_count=w["max_count"][0])
    want["local"], want["n_local"] = R.local_keyframes_fast(want["weights"], T["kf_bad"], neigh, parent, 80, 10)
    return dict(sc=sc, lms=lms, T=T, neigh=np.ascontiguousarray(neigh, np.int32), parent=parent, flm=flm, want=want)


def _device_frame(fa):
    import oracle
    from hyslam_amd import _native as N
    Fh, keep = oracle.make_frame_view(N.FrameView, **fa)
    bufs = [dev(np.ascontiguousarray(fa["kps"], N.KP_DTYPE)), dev(np.ascontiguousarray(fa["desc"], np.uint8)), dev(np.ascontiguousarray(fa["uR"], np.float32)),
            dev(np.ascontiguousarray(fa["kp_lm_obs"], np.int32))]
    Fd = N.FrameView.from_buffer_copy(Fh)
    Fd.kps, Fd.desc, Fd.uR, Fd.kp_lm_obs = (b.ptr for b in bufs)
    return Fd, bufs


OUT_SPEC = (("weights", np.int32, "n_kf"), ("max_slot", np.int32, 1), ("max_count", np.int32, 1), ("local", np.uint8, "n_kf"), ("n_local", np.int32, 1),
            ("frame_remove", np.uint8, "n_assoc"), ("sel", np.int32, "cap"), ("n_sel", np.int32, 1), ("lms", None, "cap"), ("match_idx", np.int32, "cap"),
            ("match_dist", np.float32, "cap"), ("n_matches", np.int32, 1))


def _outputs(sizes):
    from hyslam_amd import _native as N
    spec = [(k, N.LM_DTYPE if dt is None else np.dtype(dt), sizes.get(n, n)) for k, dt, n in OUT_SPEC]
    bufs = {k: out_buf(np.dtype(dt).itemsize * n) for k, dt, n in spec}
    return spec, bufs, N.LocalMapOut(*[bufs[k].ptr for k, _, _ in spec])


def _run_chain(ex, scene, cap, fused):
    from hyslam_amd import _native as N
    T, flm = scene["T"], scene["flm"]
    KT, keep = native_table(T, on_device=True)
    Fd, fkeep = _device_frame(scene["sc"]["frame_args"])
    pp = N.ProjParams(5.0, 100.0, 0.8, 0.5, 1.5, 1, 1, 0)                                # SearchByProjection(Frame, MapPoints, th = 5)
    d_flm, d_neigh, d_parent, d_lms = dev(flm), dev(scene["neigh"]), dev(scene["parent"]), dev(scene["lms"])
    spec, bufs, out = _outputs(dict(n_kf=KT.n_kf, n_assoc=len(flm), cap=cap))
    work = out_buf(ex.local_map_work_bytes(KT.L))
    s = hipmem.Stream()
    if fused:
        ex.local_map_search_device(KT, d_flm.ptr, len(flm), d_neigh.ptr, 10, d_parent.ptr, 80, 10, Fd, d_lms.ptr, pp, cap, out, work.ptr, s.ptr)
    else:
        q_off, d_n_ord = dev(np.array([0, len(flm)], np.int64)), out_buf(4)
        N.check(ex._h, ex._lib.hs_kf_votes_device(ex._h, C.byref(KT), 1, q_off.ptr, d_flm.ptr, None, 1, 1, out.weights, out.max_slot, out.max_count, None, None,
                                                  0, d_n_ord.ptr, s.ptr))
        ex.local_keyframes_device(KT.n_kf, out.weights, KT.kf_bad, d_neigh.ptr, 10, d_parent.ptr, 80, 10, out.local, out.n_local, s.ptr)
        ex.local_points_device(KT, out.local, d_flm.ptr, len(flm), out.frame_remove, out.sel, cap, out.n_sel, work.ptr, s.ptr)
        ex.landmark_gather_device(d_lms.ptr, KT.L, out.sel, out.n_sel, cap, out.lms, s.ptr)
        N.check(ex._h, ex._lib.hs_search_by_projection_device(ex._h, C.byref(Fd), out.lms, cap, C.byref(pp), out.match_idx, out.match_dist, out.n_matches, s.ptr))
    s.synchronize()
    read(work, np.uint8, ex.local_map_work_bytes(KT.L))
    return {k: read(bufs[k], dt, n) for k, dt, n in spec}


def test_fused_call_equals_the_five_calls_and_the_reference(matcher, scene):
    import oracle
    from test_oracle_matchers import py_search_by_projection
    ex, want, L = matcher._ex, scene["want"], len(scene["lms"])
    full = R.local_points_fast(scene["T"], want["local"], scene["flm"], L)
    n = full["n_sel"]
    assert want["n_local"] == int(((want["weights"] > 0) & (scene["T"]["kf_bad"] == 0)).sum()) + 2 and 50 < n < L and full["frame_remove"].any()
    for cap in (L, n // 2):
        fused, apart = _run_chain(ex, scene, cap, True), _run_chain(ex, scene, cap, False)
        for k, _, _ in OUT_SPEC:
            assert fused[k].tobytes() == apart[k].tobytes(), (cap, k)
        pts = R.local_points_fast(scene["T"], want["local"], scene["flm"], cap)
        for k in ("weights", "max_slot", "max_count", "local", "n_local"):
            assert np.array_equal(fused[k].reshape(np.shape(want[k])), want[k]), (cap, k)
        assert R.same(dict(frame_remove=fused["frame_remove"], sel=fused["sel"], n_sel=int(fused["n_sel"][0])), pts) is None
        gathered = R.gather(scene["lms"], pts["sel"], n, cap)
        assert fused["lms"].tobytes() == gathered.tobytes()
        ref = py_search_by_projection(scene["sc"]["frame_args"], gathered, oracle.ProjParams(5.0, 100.0, 0.8, 0.5, 1.5, 1, 1, 0))
        got = {int(j): (int(fused["match_idx"][j]), float(fused["match_dist"][j])) for j in np.nonzero(fused["match_idx"] >= 0)[0]}
        assert got == ref and int(fused["n_matches"][0]) == len(ref), cap                  # match_idx[j] belongs to landmark sel[j]
        assert len(ref) > (10 if cap == L else 4)
