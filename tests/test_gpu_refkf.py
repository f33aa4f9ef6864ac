"""GPU: the BoW search against a resident key frame and the association replay in view order (hs_search_by_bow_kf_device,
hs_frame_associate_views_device; include/hyslam_amd.h) against tests/ref_refkf.py, which tests/test_refkf_ref.py pins on the CPU.

  * hs_search_by_bow_kf_device against the dense restatement AND the literal one (ref_bow.search_by_bow over feature vectors, the std::map walk): every
    directed key-frame store (two keypoints taking one view, bad landmarks, slot -1 / past the store, an empty key frame, kf_cap truncation) and a
    frame and key frame beyond 1024 keypoints (the second trip of the one-workgroup loops); twice, same bytes
  * hs_frame_associate_views_device against the sequential LandMarkMatches model: sizes around the 64-lane wave, the 256-thread workgroup and 1024; ops
    in shuffled array order; twice, same bytes
  * the two calls one after the other leave the associations TrackReferenceKeyFrame::track has before it optimises, on every directed case that
    passes the BoW gate
  * hs_bow_transform_device feeds the search with nothing in between, on a vocabulary (through hs_vocab_from_tree and hs_vocab_upload) some of whose
    words have no positive weight
  * FrameTracker.SearchByBoWKeyFrame / AssociateLandMarks return the same
Every device output has guard bytes behind it, checked on every read."""
import numpy as np
import pytest

import hipmem
import ref_bow
import ref_refkf as RR
import ref_track as R
import refkf_cases as RC
import scenes
import track_cases as TC
from devbuf import dev, guarded, out_buf, read

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tracker(gpu):
    import hyslam_amd as HS
    return HS.FrameTracker(HS.ORBExtractor(device=0))


def device_keyframes(K):
    """-> (_native.KfFeatures, buffers); with K["weight"] the store carries the transform's weights and its nodes unmasked"""
    from hyslam_amd import _native as N
    bufs = [dev(np.ascontiguousarray(K["kf_off"], np.int64)), dev(np.ascontiguousarray(K["kps"], N.KP_DTYPE)), dev(np.ascontiguousarray(K["desc"], np.uint8)),
            dev(np.ascontiguousarray(K["node"], np.int32)), dev(np.ascontiguousarray(K["kp_lm"], np.int32))]
    if K.get("weight") is not None:
        bufs.append(dev(np.ascontiguousarray(K["weight"], np.float32)))
    return N.KfFeatures(K["n_kf"], *[b.ptr for b in bufs], *([None] if len(bufs) == 5 else [])), bufs


# ---------------------------------------------------------------- the search alone
def search_device(tracker, K, slot, kf_cap, lm_bad, L, fkps, fdesc, fnode, th_low, nnratio, fweight=None):
    from hyslam_amd import _native as N
    n = len(fkps)
    KF, keep = device_keyframes(K)
    d_bad = dev(np.ascontiguousarray(lm_bad, np.uint8))
    KT = N.KfTable(L, 0, None, None, None, d_bad.ptr, None, None, None)
    ins = dev(np.ascontiguousarray(fkps, N.KP_DTYPE)), dev(np.ascontiguousarray(fdesc, np.uint8)), dev(np.ascontiguousarray(fnode, np.int32)), dev(np.array([slot], np.int32))
    d_w = None if fweight is None else dev(np.ascontiguousarray(fweight, np.float32))
    outs = out_buf(kf_cap * 4), out_buf(n * 4), out_buf(n * 4), out_buf(4)
    st = hipmem.Stream()
    tracker.search_by_bow_kf_device(KF, ins[3].ptr, KT, ins[0].ptr, ins[1].ptr, ins[2].ptr, d_w.ptr if d_w else None, n, th_low, nnratio, outs[0].ptr, kf_cap, outs[1].ptr, outs[2].ptr,
                                    outs[3].ptr, None, st.ptr)
    st.synchronize()
    return read(outs[0], np.int32, kf_cap), read(outs[1], np.int32, n), read(outs[2], np.int32, n), int(read(outs[3], np.int32, 1)[0])


def check_search(tracker, K, slot, kf_cap, lm_bad, L, fkps, fdesc, fword, fweight, fnode, th_low, nnratio, tag):
    masked = np.where(np.asarray(fweight) > 0, fnode, -1).astype(np.int32)          # the public call takes the feature vector as the node array alone
    got = search_device(tracker, K, slot, kf_cap, lm_bad, L, fkps, fdesc, masked, th_low, nnratio)
    want = RR.search_by_bow_kf_dense(K, slot, kf_cap, L, lm_bad, fkps, fdesc, masked, None, th_low, nnratio)
    for g, w, what in zip(got, want, ("match_kf", "op_view", "op_lm", "n_matches")):
        assert np.array_equal(g, w), (tag, what)
    bow, internal, nm = RR.search_by_bow_kf(K, slot, kf_cap, lm_bad, fkps, fdesc, fword, fweight, fnode, th_low, nnratio)
    assert nm == got[3] and internal == {int(j): int(f) for j, f in enumerate(got[0]) if f >= 0}, (tag, "literal")
    assert bow == {int(f): int(got[2][f]) for f in np.nonzero(got[1] >= 0)[0]}, (tag, "literal")
    again = search_device(tracker, K, slot, kf_cap, lm_bad, L, fkps, fdesc, masked, th_low, nnratio)
    for a, g in zip(again, got):
        assert np.asarray(a).tobytes() == np.asarray(g).tobytes(), (tag, "second call")
    raw = search_device(tracker, K, slot, kf_cap, lm_bad, L, fkps, fdesc, fnode, th_low, nnratio, fweight)      # the transform's node and weight as they are
    for a, g in zip(raw, got):
        assert np.asarray(a).tobytes() == np.asarray(g).tobytes(), (tag, "weights on the device")
    return got


@pytest.mark.parametrize("name", ["two_take_one_view", "bad_kf_landmark", "slot_minus_one", "slot_past_the_store", "empty_keyframe", "kf_cap_truncates", "mono"])
def test_search_by_bow_kf_directed(tracker, name):
    c, _, (_, rk, _) = RC.directed(name)
    fr, rp = c["frame"], c["rp"]
    got = check_search(tracker, c["K"], c["kf_slot"], c["kf_cap"], c["T"]["lm_bad"], len(c["lms"]), fr["kps"], fr["desc"], rk["bow_word"], rk["bow_weight"],
                       rk["bow_node"], rp.th_low, rp.nnratio, name)
    assert np.array_equal(got[0], rk["match_kf"]) and got[3] == rk["result"]["n_bow"][0]
    if name == "kf_cap_truncates":                                       # every key frame of the store through one capacity: longer, exact, shorter, empty
        for slot in (0, 1, 2):
            check_search(tracker, c["K"], slot, 40, c["T"]["lm_bad"], len(c["lms"]), fr["kps"], fr["desc"], rk["bow_word"], rk["bow_weight"], rk["bow_node"],
                         rp.th_low, rp.nnratio, (name, slot))


def test_search_by_bow_kf_beyond_one_pass(tracker):
    """1100 frame keypoints and a key frame of 1030 (in a store whose other key frame has 3): the one-workgroup kernel's loops take a second trip, the
    per-keypoint kernel more than 17 lane strides; ties and near twins so that the histogram removes matches and several keypoints take one view"""
    rng = np.random.default_rng(77)
    n, nk, L = 1100, 1030, 1500
    tree = scenes.flat_tree(rng, 3, lambda i, lv, m: 3, zero_weight=0.05)
    fdesc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    fkps = np.zeros(n, TC.KP_DTYPE)
    fkps["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    src = rng.integers(0, n, nk)                                         # with repeats: twins
    total = 3 + nk
    K = dict(n_kf=2, kf_off=np.array([0, 3, total], np.int64), kps=np.zeros(total, TC.KP_DTYPE), desc=rng.integers(0, 256, (total, 32), dtype=np.uint8),
             kp_lm=np.full(total, -1, np.int32))
    K["desc"][3:] = scenes.flip_bits(rng, fdesc[src], rng.integers(0, 14, nk))
    K["kps"]["angle"][3:] = ((fkps["angle"][src] + 300 + rng.normal(0, 4, nk) + (rng.random(nk) < 0.15) * rng.uniform(0, 360, nk)) % 360).astype(np.float32)
    K["kp_lm"][3:] = np.where(rng.random(nk) < 0.9, rng.permutation(L)[:nk], -1)
    w, wt, nd = ref_bow.bow_transform(tree, K["desc"], 2)
    K["node"] = np.where(wt > 0, nd, -1).astype(np.int32)
    lm_bad = (rng.random(L) < 0.05).astype(np.uint8)
    fw, fwt, fnd = ref_bow.bow_transform(tree, fdesc, 2)
    got = check_search(tracker, K, 1, nk, lm_bad, L, fkps, fdesc, fw, fwt, fnd, 50.0, 0.8, "beyond one pass")
    live = got[0][got[0] >= 0]
    assert got[3] > 500 and len(np.unique(live)) < len(live) and (got[0][1024:] >= 0).any() and (got[1][1024:] >= 0).any()


# ---------------------------------------------------------------- the replay alone
def associate_views_device(tracker, s, order=None, stream=None):
    """stream: anything with .ptr and .synchronize() (default: a stream of its own)"""
    n, L = len(s["kp_lm"]), s["L"]
    ov, ol = (s["op_view"], s["op_lm"]) if order is None else (s["op_view"][order], s["op_lm"][order])
    d_lm, d_outl, d_nm = guarded(s["kp_lm"]), guarded(s["kp_outl"]), guarded(np.array([s["n_matches"]], np.int32))
    d_ov, d_ol = dev(ov), dev(ol)
    nbytes = tracker.track_refkf_work_bytes(n, 0, L)
    work = out_buf(nbytes)
    st = stream or hipmem.Stream()
    tracker.frame_associate_views_device(n, L, d_lm.ptr, d_outl.ptr, d_nm.ptr, d_ov.ptr, d_ol.ptr, work.ptr, st.ptr)
    st.synchronize()
    read(work, np.uint8, nbytes)
    return read(d_lm, np.int32, n), read(d_outl, np.uint8, n), int(read(d_nm, np.int32, 1)[0])


@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 130, 255, 256, 257, 1023, 1024, 1025])
def test_associate_views_against_the_sequential_model(tracker, n):
    for seed in range(3):
        s = RC.replay_state(88000 + 1000 * seed + n, n)
        want = RR.replay_views_sequential(R.MapMatches.from_dense(s["kp_lm"], s["kp_outl"], s["n_matches"]), s["op_view"], s["op_lm"], n, s["L"]).dense(n)
        got = associate_views_device(tracker, s)
        for w, g, what in zip(want, got, ("kp_lm", "kp_outl", "n_matches")):
            assert np.array_equal(w, g), (what, n, seed)
        again = associate_views_device(tracker, s, np.random.default_rng(seed).permutation(n))       # array order does not matter, and the bytes repeat
        for a, g in zip(again, got):
            assert np.asarray(a).tobytes() == np.asarray(g).tobytes()


def test_associate_views_by_hand(tracker):
    """view order, by hand.  View 0 takes landmark 2 from view 3 (idx_old = 3: erased, its flag stays, n_matches unchanged); view 1 holds landmark 1 twice
    over with view 2 and takes it again: the first holder is itself, nothing is erased; view 3, emptied by view 0's op, takes landmark 0 as a FRESH
    insert whose stale `true` flag survives; in landmark order (the motion stage's replay) op 0 would have run first, onto an occupied view"""
    s = dict(kp_lm=np.array([-1, 1, 1, 2], np.int32), kp_outl=np.array([0, 2, 1, 2], np.uint8), n_matches=3, L=4,
             op_view=np.array([3, 0, 1, -1], np.int32), op_lm=np.array([0, 2, 1, -1], np.int32))
    kp_lm, outl, nm = associate_views_device(tracker, s)
    assert kp_lm.tolist() == [2, 1, 1, 0] and outl.tolist() == [1, 1, 1, 2] and nm == 4
    other = R.replay_sequential(R.MapMatches.from_dense(s["kp_lm"], s["kp_outl"], 3), s["op_view"], s["op_lm"], 4, 4).dense(4)
    assert other[1].tolist() != outl.tolist() or other[2] != nm


# ---------------------------------------------------------------- the transform feeds the search
def tree_dict(T):
    """a _native.VocabTree (host arrays) as the dict ref_bow works on"""
    import ctypes as C
    arr = lambda p, ct, n: np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(n,)).copy()
    n = T.n_nodes
    return dict(levels=T.levels, n_nodes=n, child_begin=arr(T.child_begin, C.c_int32, n), child_count=arr(T.child_count, C.c_int32, n),
                desc=arr(T.desc, C.c_uint8, n * 32).reshape(n, 32), word_id=arr(T.word_id, C.c_int32, n), weight=arr(T.weight, C.c_float, n),
                orig_id=arr(T.orig_id, C.c_int32, n) if T.orig_id else None)


@pytest.mark.parametrize("name", ["plain", "two_take_one_view", "mono"])
def test_transform_feeds_the_search_on_the_device(tracker, name):
    """ComputeBoW into SearchByBoW with nothing in between: the case's synthetic vocabulary (a share of its words has no positive weight) goes through
    hs_vocab_from_tree and hs_vocab_upload, hs_bow_transform_device writes node and weight for the frame and for the whole key-frame store, and the
    search reads those buffers as they are.  Against the literal restatement on the vocabulary object's own tree, whose feature vectors leave the
    weightless keypoints out as DBoW2 does"""
    import ctypes as C
    from hyslam_amd import _native as N
    from hyslam_amd.distributed import DeviceVocabulary
    c, _, _ = RC.directed(name)
    ex, fr, rp, K, L = tracker._ex, c["frame"], c["rp"], c["K"], len(c["lms"])
    v, T = C.c_void_p(), N.VocabTree()
    assert ex._lib.hs_vocab_from_tree(C.byref(scenes.tree_struct(N.VocabTree, c["tree"])), 3, C.byref(v)) == N.HS_OK
    try:
        assert ex._lib.hs_vocab_get_tree(v, C.byref(T)) == N.HS_OK
        tree = tree_dict(T)
        voc = DeviceVocabulary(ex, T, c["levelsup"])
        n, total = len(fr["kps"]), len(K["kps"])
        st = hipmem.Stream()
        d_fdesc, d_kdesc = dev(fr["desc"]), dev(K["desc"])
        f_out = out_buf(n * 4), out_buf(n * 4), out_buf(n * 4)
        k_out = out_buf(total * 4), out_buf(total * 4), out_buf(total * 4)
        voc.transform_device(d_fdesc.ptr, 0, n, f_out[0].ptr, f_out[1].ptr, f_out[2].ptr, st.ptr)
        voc.transform_device(d_kdesc.ptr, 0, total, k_out[0].ptr, k_out[1].ptr, k_out[2].ptr, st.ptr)
        keep = [dev(np.ascontiguousarray(K["kf_off"], np.int64)), dev(np.ascontiguousarray(K["kps"], N.KP_DTYPE)), dev(np.ascontiguousarray(K["kp_lm"], np.int32))]
        KF = N.KfFeatures(K["n_kf"], keep[0].ptr, keep[1].ptr, d_kdesc.ptr, k_out[2].ptr, keep[2].ptr, k_out[1].ptr)
        d_bad, d_kps, d_slot = dev(c["T"]["lm_bad"]), dev(np.ascontiguousarray(fr["kps"], N.KP_DTYPE)), dev(np.array([c["kf_slot"]], np.int32))
        KT = N.KfTable(L, 0, None, None, None, d_bad.ptr, None, None, None)
        outs = out_buf(c["kf_cap"] * 4), out_buf(n * 4), out_buf(n * 4), out_buf(4)
        tracker.search_by_bow_kf_device(KF, d_slot.ptr, KT, d_kps.ptr, d_fdesc.ptr, f_out[2].ptr, f_out[1].ptr, n, rp.th_low, rp.nnratio, outs[0].ptr, c["kf_cap"],
                                        outs[1].ptr, outs[2].ptr, outs[3].ptr, None, st.ptr)
        st.synchronize()
        fw, fwt, fnd = ref_bow.bow_transform(tree, fr["desc"], c["levelsup"])
        kw, kwt, knd = ref_bow.bow_transform(tree, K["desc"], c["levelsup"])
        assert np.array_equal(read(f_out[2], np.int32, n), fnd) and read(f_out[1], np.float32, n).tobytes() == fwt.tobytes()
        assert np.array_equal(read(k_out[2], np.int32, total), knd) and read(k_out[1], np.float32, total).tobytes() == kwt.tobytes()
        a, b = K["kf_off"][c["kf_slot"]], K["kf_off"][c["kf_slot"] + 1]
        assert (fwt <= 0).any() and (kwt[a:b] <= 0).any()                 # weightless words on both sides, on keypoints that would otherwise match
        Kref = dict(K, node=np.where(kwt > 0, knd, -1).astype(np.int32))
        bow, internal, nm = RR.search_by_bow_kf(Kref, c["kf_slot"], c["kf_cap"], c["T"]["lm_bad"], fr["kps"], fr["desc"], fw, fwt, fnd, rp.th_low, rp.nnratio)
        match_kf, op_view, op_lm = read(outs[0], np.int32, c["kf_cap"]), read(outs[1], np.int32, n), read(outs[2], np.int32, n)
        assert int(read(outs[3], np.int32, 1)[0]) == nm > 10 and internal == {int(j): int(f) for j, f in enumerate(match_kf) if f >= 0}
        assert bow == {int(f): int(op_lm[f]) for f in np.nonzero(op_view >= 0)[0]}
        # and the weights matter: with every keypoint in its node the weightless ones take part and the count is another
        loose = RR.search_by_bow_kf_dense(dict(K, node=knd), c["kf_slot"], c["kf_cap"], L, c["T"]["lm_bad"], fr["kps"], fr["desc"], fnd, None, rp.th_low, rp.nnratio)
        assert loose[3] != nm, name
        voc.close()
    finally:
        ex._lib.hs_vocab_destroy(v)


# ---------------------------------------------------------------- the two together
@pytest.mark.parametrize("name", [k for k, (_, vv, _) in RC.DIRECTED.items() if vv == 0])
def test_search_then_replay_is_the_reference_frame(tracker, name):
    """search, then replay on the case's entry state: the associations of the reference's frame after associateLandMarks (literal restatement on the
    maps); a landmark the frame holds on another view moves, an occupied view is overwritten; through the numpy-level methods"""
    c, _, (_, rk, _) = RC.directed(name)
    fr, rp, s0 = c["frame"], c["rp"], c["state0"]
    node = np.where(rk["bow_weight"] > 0, rk["bow_node"], -1).astype(np.int32)
    matches, match_kf, nm = tracker.SearchByBoWKeyFrame(c["K"], c["kf_slot"], c["T"], fr["kps"], fr["desc"], node, rp.th_low, rp.nnratio, c["kf_cap"])
    assert tracker.SearchByBoWKeyFrame(c["K"], c["kf_slot"], c["T"], fr["kps"], fr["desc"], rk["bow_node"], rp.th_low, rp.nnratio, c["kf_cap"],
                                       weight=rk["bow_weight"])[0] == matches                      # the transform's arrays as they are
    bow, internal, want_n = RR.search_by_bow_kf(c["K"], c["kf_slot"], c["kf_cap"], c["T"]["lm_bad"], fr["kps"], fr["desc"], rk["bow_word"], rk["bow_weight"],
                                                rk["bow_node"], rp.th_low, rp.nnratio)
    assert matches == bow and nm == want_n == rk["result"]["n_bow"][0] and np.array_equal(match_kf, rk["match_kf"])
    got = tracker.AssociateLandMarks(s0[0], s0[1], s0[2], matches, len(c["lms"]))
    want = RR.associate_landmarks(R.MapMatches.from_dense(*s0), bow).dense(len(fr["kps"]))
    for g, w, what in zip(got, want, ("kp_lm", "kp_outl", "n_matches")):
        assert np.array_equal(g, w), (name, what)
    if rk["status"] == RR.REFKF_OK:                                      # the state the dense chain optimises from
        for g, w in zip(got, rk["after_associate"]):
            assert np.array_equal(g, w), name


def test_refusals(tracker):
    """what the two entry points refuse on the host: a missing store, kf_cap < 1, a frame without keypoints, a missing output or work area"""
    import ctypes as C
    from hyslam_amd import _native as N
    c, _, (_, rk, _) = RC.directed("plain")
    ex, fr = tracker._ex, c["frame"]
    n = len(fr["kps"])
    KF, keep = device_keyframes(c["K"])
    d_bad = dev(c["T"]["lm_bad"])
    KT = N.KfTable(len(c["lms"]), 0, None, None, None, d_bad.ptr, None, None, None)
    ins = dev(np.ascontiguousarray(fr["kps"], N.KP_DTYPE)), dev(fr["desc"]), dev(np.where(rk["bow_weight"] > 0, rk["bow_node"], -1).astype(np.int32)), dev(np.array([1], np.int32))
    outs = out_buf(80 * 4), out_buf(n * 4), out_buf(n * 4), out_buf(4)

    def search(K=KF, n=n, kf_cap=80, match=outs[0].ptr, slot=ins[3].ptr):
        return ex._lib.hs_search_by_bow_kf_device(ex._h, None if K is None else C.byref(K), slot, C.byref(KT), ins[0].ptr, ins[1].ptr, ins[2].ptr, None, n, 50.0, 0.7, match,
                                                  kf_cap, outs[1].ptr, outs[2].ptr, outs[3].ptr, None, None)
    for kw in (dict(K=None), dict(n=0), dict(n=65536), dict(kf_cap=0), dict(match=None), dict(slot=None)):
        assert search(**kw) == N.HS_ERR_INVALID, kw
    st = guarded(c["state0"][0]), guarded(c["state0"][1]), guarded(np.array([0], np.int32))
    assert ex._lib.hs_frame_associate_views_device(ex._h, n, 160, st[0].ptr, st[1].ptr, st[2].ptr, outs[1].ptr, outs[2].ptr, None, None) == N.HS_ERR_INVALID
    assert ex._lib.hs_frame_associate_views_device(ex._h, -1, 160, st[0].ptr, st[1].ptr, st[2].ptr, outs[1].ptr, outs[2].ptr, outs[0].ptr, None) == N.HS_ERR_INVALID
    assert search() == N.HS_OK                                           # the handle is as good as before
    ex.synchronize()
    assert int(read(outs[3], np.int32, 1)[0]) == rk["result"]["n_bow"][0]
