"""GPU: every `*_device` entry point does ALL of its work in the order of the caller's stream.  tests/stream_order.py holds the stream
back with a delay, lets the real inputs arrive behind it by device-to-device copies (the buffers hold a valid DECOY until then), snapshots the outputs
on the stream right behind the call, overwrites them with 0xEE behind the snapshot, waits for that one stream and reads.  Per call: the snapshot is the
reference's result for the real inputs (as exact as the module's own GPU test: everything byte for byte but Tcw_d, within the golden file's tau), no
defined byte holds 0x55 or the decoy's result, the outputs read 0xEE afterwards, and the delay had not ended when the host finished enqueueing (or the
run is repeated with twice the delay).  The pairs come from tests/stream_order_cases.py (checked on the CPU by tests/test_stream_order_cases.py).

Calls that may wait on the host, stated per step (`waits`) and exempt from the not-ready condition, never from the bytes:
  - the first extractor / stereo front end call of a fresh handle configures its workspace (allocations);
  - hs_records_bow_match_device when the vocabulary's scratch grows (hipDeviceSynchronize, then reallocation);
  - the first hs_place_query_*_device after an add uploads the walk order (hipStreamSynchronize(stream), then a blocking copy).
hs_place_db_add_device would wait when the database's storage grows: the scenes add 30 key frames through the host form first, so it does not.

Left out:
  - hs_track_frame_device, hs_track_keyframe_device, hs_landmark_update_entries_device, hs_search_by_bow_kf_device and hs_frame_associate_views_device:
    tests/test_gpu_chain_run.py runs them back to back on a caller stream with snapshots by device-to-device copies;
  - the single-stage tracking and key-frame calls (hs_track_motion_model_device, hs_track_local_map_device, hs_keyframe_*_device, hs_pose_views_device,
    hs_frame_associate_device, hs_frame_views_device, hs_track_discard_device, hs_local_map_search_posed_device): the same launchers as the fused calls above;
  - the ticket API (hs_orb_submit_batch / hs_orb_wait): it owns its streams; tests/test_gpu_ingest.py."""
import ctypes as C

import numpy as np
import pytest

import hipmem
import oracle
import stream_order as SO
import stream_order_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def nothing_more_after_a_device_error():
    """a HIP error that a test left behind (a fault is sticky) ends the module's run: nothing more is started on that device"""
    yield
    rc = hipmem.hip().hipDeviceSynchronize()
    if rc != 0:
        pytest.exit("hipError %d after this test: nothing more is started on the device" % rc, returncode=3)


@pytest.fixture(scope="module")
def HS(gpu):
    import hyslam_amd as HS
    return HS


@pytest.fixture(scope="module")
def delay_ex(HS):
    """the handle whose hs_debug_stream_copy is the delay: never the handle under test"""
    return HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=500), device=0)


@pytest.fixture(scope="module")
def ex(HS):
    """the warmed handle of the calls that configure nothing"""
    return HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=S.NF), device=0)


@pytest.fixture(scope="module")
def cases():
    return {(c.kind, c.name): c for c in S.single_cases(probe_cap())}


_CAP = []


def probe_cap():
    """hs_orb_max_keypoints() of a handle configured for the scenes' 640 x 480 frames: the row stride of the extractor's outputs"""
    if not _CAP:
        import hyslam_amd as HS
        probe = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=S.NF), device=0)
        probe.reserve(S.W, S.H, 2)
        _CAP.append(probe.max_keypoints())
        probe.close()
    return _CAP[0]


# ---------------------------------------------------------------- one Case -> one Step
def kf_table(N, c, p):
    return N.KfTable(c.args["L"], c.args["n_kf"], *[p["T." + k] for k in S.TABLE_KEYS])


def frame_view(N, fa, p, pose=True):
    Fh, _ = oracle.make_frame_view(N.FrameView, **fa)
    F = N.FrameView.from_buffer_copy(Fh)
    F.kps, F.desc, F.uR, F.kp_lm_obs = p.get("F.kps"), p.get("F.desc"), p.get("F.uR"), p.get("F.kp_lm_obs")
    if not pose:                                                  # not read: the pose comes from the device
        F.Rcw[:] = [7.0] * 9; F.tcw[:] = [7.0] * 3; F.Ow[:] = [7.0] * 3
    return F


def stereo_params(N, sp):
    return N.StereoParams(sp["fx"], sp["mbf"], sp["n_rows"], sp["th_high"], sp["th_low"], sp["size_ref"])


def check_match_dist(c):
    """match_dist where match_idx >= 0 (a dropped entry keeps its distance, as the device form documents), bit for bit"""
    def check(got, which):
        w = 0 if which == "real" else 1
        idx, dist = c.aux["match_idx"][w], c.aux["match_dist"][w]
        g = got["match_dist"].view(np.float32)
        assert g[idx >= 0].tobytes() == dist[idx >= 0].tobytes(), (c, "match_dist")
    return check


def check_pose_result(N, c):
    """the result record as tests/test_gpu_poseopt.py compares it: the integers exactly, Tcw_d within the golden file's tau, Tcw the float of Tcw_d
    and within one float ulp of the reference's"""
    def check(got, which):
        ref, tau = c.aux["ref"][0 if which == "real" else 1], c.aux["tau"]
        r = got["results"].view(N.POSE_RESULT_DTYPE)[0]
        dev = float(np.abs(r["Tcw_d"].reshape(4, 4) - ref["Tcw_d"]).max())
        print("%r: |Tcw_d - reference| %.3e (tau %.3e)" % (c, dev, tau))
        assert [int(r[k]) for k in ("n_good", "n_edges", "rounds", "status")] == [int(ref[k]) for k in ("n_good", "n_edges", "rounds", "status")]
        assert dev <= tau
        assert r["Tcw"].tobytes() == r["Tcw_d"].astype(np.float32).tobytes()
        assert np.abs(r["Tcw"].view(np.int32).astype(np.int64) - ref["Tcw"].reshape(16).view(np.int32).astype(np.int64)).max() <= 1
    return check


def step(c, ex, voc=None, db=None, waits=None):
    """the Step of Case c on handle ex (voc: the device vocabulary, db: the place recogniser)"""
    from hyslam_amd import _native as N
    from hyslam_amd import distributed as D
    a, lib, h = c.args, ex._lib, ex._h
    work, check = {}, None
    if c.kind == "landmark_best_descriptors":
        call = lambda p, s: ex.landmark_best_descriptors_device(p["offsets"], a["L"], p["desc"], p["best"], p["median"], stream=s)
    elif c.kind == "kf_votes":
        call = lambda p, s: N.check(h, lib.hs_kf_votes_device(h, C.byref(kf_table(N, c, p)), a["Q"], p["q_offsets"], p["q_lm"], p["q_self_id"], a["count_bad_kf"], a["th"],
                                                              p["weights"], p["max_slot"], p["max_count"], p["ordered_slot"], p["ordered_weight"], a["cap"], p["n_ordered"], s))
    elif c.kind == "kf_redundancy":
        call = lambda p, s: N.check(h, lib.hs_kf_redundancy_device(h, C.byref(kf_table(N, c, p)), a["C"], p["cand_slot"], p["cand_th_depth"], p["cand_offsets"], p["item_lm"],
                                                                   p["item_octave"], p["item_depth"], a["is_mono"], a["th_obs"], a["frac"], p["n_mps"], p["n_redundant"],
                                                                   p["cull"], s))
    elif c.kind == "local_keyframes":
        call = lambda p, s: ex.local_keyframes_device(a["n_kf"], p["weights"], p["kf_bad"], p["neigh"], a["neigh_cap"], p["parent"], a["n_max"], a["n_neighbor"], p["local"],
                                                      p["n_local"], s)
    elif c.kind == "local_points":
        work = dict(work=ex.local_points_work_bytes(a["L"]))
        call = lambda p, s: ex.local_points_device(kf_table(N, c, p), p["local"], p["frame_lm"], a["n_assoc"], p["frame_remove"], p["sel"], a["cap"], p["n_sel"], p["work"], s)
    elif c.kind == "landmark_gather":
        call = lambda p, s: ex.landmark_gather_device(p["lms"], a["L"], p["sel"], p["n_sel"], a["cap"], p["out"], s)
    elif c.kind == "local_map_search":
        work, check = dict(work=ex.local_map_work_bytes(a["L"])), check_match_dist(c)
        call = lambda p, s: ex.local_map_search_device(kf_table(N, c, p), p["frame_lm"], a["n_assoc"], p["neigh"], a["neigh_cap"], p["parent"], 80, 10, frame_view(N, a["frame"], p),
                                                       p["map_lms"], N.ProjParams(*a["proj"]), a["cap"], N.LocalMapOut(*[p[k] for k in S.LOCAL_MAP_OUT]), p["work"], s)
    elif c.kind == "extract_batch":
        call = lambda p, s: ex.extract_batch_device(p["imgs"], a["batch"], a["w"], a["h"], a["w"], a["w"] * a["h"], p["kps"], p["desc"], p["n"], a["cap"], s)
    elif c.kind == "stereo_frontend":
        call = lambda p, s: ex.stereo_frontend_batch_device(p["left"], p["right"], a["pairs"], a["w"], a["h"], a["w"], a["w"] * a["h"], p["kpsL"], p["descL"], p["nL"],
                                                            p["kpsR"], p["descR"], p["nR"], a["cap"], stereo_params(N, a["sp"]), p["uRight"], p["depth"], s)
    elif c.kind == "stereo_match":
        call = lambda p, s: ex.stereo_match_batch_device(p["kpsL"], p["descL"], p["nL"], p["kpsR"], p["descR"], p["nR"], a["pairs"], a["cap"], stereo_params(N, a["sp"]),
                                                         p["uRight"], p["depth"], s)
    elif c.kind == "preprocess":
        call = lambda p, s: ex.preprocess_device(p["src"], a["w"], a["h"], a["row"], a["h"] * a["row"], a["batch"], a["cn"], a["rgb"], a["scale"], p["grey"], a["gpitch"],
                                                 a["oh"] * a["gpitch"], s)
    elif c.kind == "projection":
        check = check_match_dist(c)
        call = lambda p, s: N.check(h, lib.hs_search_by_projection_device(h, C.byref(frame_view(N, a["frame"], p)), p["lms"], a["L"], C.byref(N.ProjParams(*a["proj"])),
                                                                          p["match_idx"], p["match_dist"], p["n_matches"], s))
    elif c.kind == "projection_posed":
        check = check_match_dist(c)
        call = lambda p, s: N.check(h, lib.hs_search_by_projection_posed_device(h, C.byref(frame_view(N, a["frame"], p, pose=False)), p["pose"], p["lms"], a["L"],
                                                                                C.byref(N.ProjParams(*a["proj"])), p["match_idx"], p["match_dist"], p["n_matches"], s))
    elif c.kind == "pose_edges":
        call = lambda p, s: ex.pose_edges_device(frame_view(N, a["frame"], p), p["lms"], a["L"], p["kp_lm"], p["edges"], a["cap"], p["n_edges"], sigma_ref=a["sigma_ref"], stream=s)
    elif c.kind == "pose_optimize":
        check = check_pose_result(N, c)
        call = lambda p, s: ex.pose_optimize_device(1, p["problems"], p["edges"], p["outlier"], p["results"], d_n_edges=p["n_edges"], edge_cap=a["cap"], stream=s)
    elif c.kind == "hamming_knn2":
        call = lambda p, s: N.check(h, lib.hs_hamming_knn2_device(h, p["q"], a["nq"], p["t"], a["nt"], p["best_idx"], p["best_dist"], p["second_dist"], s))
    elif c.kind == "records_knn2":
        call = lambda p, s: D.records_knn2_device(ex, p["records"], a["stride"], a["world"], a["rank"], a["cap"], p["best_idx"], p["best_dist"], p["second_dist"], s)
    elif c.kind == "records_bow_match":
        call = lambda p, s: voc.records_bow_match_device(p["records"], a["stride"], a["world"], a["rank"], a["cap"], a["thr"], a["ratio"], a["rot"], p["match12"], p["n_matches"], s)
    elif c.kind == "bow_transform":
        call = lambda p, s: voc.transform_device(p["desc"], p["n"], a["n_max"], p["word"], p["weight"], p["node"], s)
    elif c.kind == "bow_vector":
        call = lambda p, s: N.check(h, lib.hs_bow_vector_device(h, p["word"], p["weight"], p["n"], a["n_max"], p["out_word"], p["out_value"], p["m"], s))
    elif c.kind == "place_add":
        def call(p, s):
            assert db.add_device(a["key"], p["word"], p["value"], p["m"], a["m_max"], s) == a["slot"]
    elif c.kind == "place_query_reloc":
        call = lambda p, s: N.check(h, lib.hs_place_query_reloc_device(db._db, p["qword"], p["qvalue"], p["qm"], a["qm_max"], p["neigh"], p["cand"], a["slots"], p["n_cand"],
                                                                       p["words"], p["score"], p["acc"], p["best"], s))
    elif c.kind == "place_query_loop":
        call = lambda p, s: N.check(h, lib.hs_place_query_loop_device(db._db, p["qword"], p["qvalue"], p["qm"], a["qm_max"], p["exclude"], a["min_score"], p["neigh"], p["cand"],
                                                                      a["slots"], p["n_cand"], p["words"], p["score"], p["acc"], p["best"], s))
    else:
        raise KeyError(c.kind)
    return SO.Step(repr(c), c.inputs, c.outputs, call, c.expect, work=work, check=check, link=getattr(c, "link", None), prefill=getattr(c, "prefill", None), waits=waits)


def run_and_check(delay_ex, scene, tag):
    for i, (steps, got, after) in enumerate(SO.run(delay_ex, scene, tag=tag)):
        SO.check(steps, got, after, "%s [caller stream %d]" % (tag, i))


# ---------------------------------------------------------------- the calls that configure nothing: one call per scene on the warmed handle
PLAIN = [("landmark_best_descriptors", "small"), ("landmark_best_descriptors", "large"), ("kf_votes", "lds"), ("kf_votes", "global"), ("kf_redundancy", "five"),
         ("local_keyframes", "129"), ("local_points", "3blocks+1"), ("landmark_gather", "37of64"), ("local_map_search", "640x480"), ("stereo_match", "3 pairs"),
         ("preprocess", "333x201x3"), ("projection", "local map"), ("projection_posed", "local map"), ("pose_edges", "640x480"), ("pose_optimize", "n257"),
         ("hamming_knn2", "321x517"), ("records_knn2", "set 5"), ("bow_vector", "n_max 5000"), ("bow_vector", "n_max 300")]


@pytest.mark.parametrize("kind,name", PLAIN, ids=["%s-%s" % kn for kn in PLAIN])
def test_plain_call(ex, delay_ex, cases, kind, name):
    """the temporaries of the matchers come from the handle's scratch arena: one call outside the harness first, so that the arena does not grow (and
    drain the stream) under the delay"""
    c = cases[kind, name]
    st, s0 = step(c, ex), hipmem.Stream()
    bufs = {k: hipmem.DevBuf.from_numpy(SO._raw(d)) for k, (r, d) in c.inputs.items()}
    bufs.update({k: hipmem.DevBuf(n) for k, n in list(c.outputs.items()) + list(st.work.items())})
    st.call({k: b.ptr for k, b in bufs.items()}, s0.ptr)          # the decoy, into buffers of its own
    s0.synchronize()
    run_and_check(delay_ex, lambda: [step(c, ex)], repr(c))


def test_pose_edges_then_optimize_with_the_count_on_the_device(ex, delay_ex, cases):
    """the two pose calls back to back on one stream, each with late inputs of its own; the optimiser reads its edge count from the device"""
    e = cases["pose_edges", "640x480"]
    run_and_check(delay_ex, lambda: [step(e, ex), step(cases["pose_optimize", "n257"], ex)], "pose edges, pose optimise")


# ---------------------------------------------------------------- the extractor: split x lanes, a fresh handle then the same handle warmed
@pytest.mark.parametrize("lanes", [2, 1])
@pytest.mark.parametrize("split", ["1", "0"])
def test_extract_batch(HS, delay_ex, monkeypatch, split, lanes):
    """2 frames of 640 x 480.  HS_EXTRACT_SPLIT=1: level 0's FAST and quadtree go to the handle's second stream behind ev_sfork and are joined before
    describe; set_lanes(2): the second frame goes to the child handle's stream behind ev_fork / ev_join.  The first call of the fresh handle allocates
    its workspace under way (it may wait: stated), the second call on the same handle, with other frames, waits for nothing"""
    monkeypatch.setenv("HS_EXTRACT_SPLIT", split)                  # read when the handle is created
    cap = probe_cap()
    first, second = S.extract_case(cap), S.extract_case(cap, seeds=(9, 10))
    made = []

    def scene():
        fresh = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=S.NF), device=0)
        fresh.set_lanes(lanes)
        made.append(fresh)
        assert fresh.max_keypoints() <= cap
        return [step(first, fresh, waits="a fresh handle configures its workspace"), step(second, fresh)]
    run_and_check(delay_ex, scene, "extract split=%s lanes=%d" % (split, lanes))
    for e in made:
        e.close()


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_stereo_frontend(HS, delay_ex, monkeypatch, fuse):
    """2 pairs of 640 x 480: extraction of four frames in one launch sequence, then the matcher; HS_STEREO_FUSE=1 bins the right keypoints inside the
    describe launch, 0 with a launch of its own.  The handle is configured (hs_orb_reserve) and has run the call once before the delay"""
    monkeypatch.setenv("HS_STEREO_FUSE", fuse)                     # read when the handle is created
    fe = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=S.NF), device=0)
    fe.reserve(S.W, S.H, 4)
    cap = fe.max_keypoints()
    c = S.stereo_frontend_case(cap)
    warm, s0 = step(c, fe), hipmem.Stream()
    bufs = {k: hipmem.DevBuf.from_numpy(SO._raw(d)) for k, (r, d) in c.inputs.items()}
    bufs.update({k: hipmem.DevBuf(n) for k, n in c.outputs.items()})
    warm.call({k: b.ptr for k, b in bufs.items()}, s0.ptr)
    s0.synchronize()
    run_and_check(delay_ex, lambda: [step(c, fe)], "stereo front end fuse=%s" % fuse)
    fe.close()


# ---------------------------------------------------------------- the vocabulary: a call that grows its scratch, then a smaller one
@pytest.fixture()
def vocabulary(ex):
    """a vocabulary uploaded anew for every test: its record-matcher scratch starts empty"""
    from hyslam_amd import _native as N
    from hyslam_amd import distributed as D
    import scenes
    e = S.vocab_tree()
    voc = D.DeviceVocabulary(ex, scenes.tree_struct(N.VocabTree, e["tree"]), S.LEVELSUP, keepalive=e["tree"])
    yield voc
    voc.close()


def test_bow_transform_large_then_small(ex, delay_ex, cases, vocabulary):
    run_and_check(delay_ex, lambda: [step(cases["bow_transform", "n_max 900"], ex, voc=vocabulary), step(cases["bow_transform", "n_max 200"], ex, voc=vocabulary)],
                  "bow transform 900, 200")


def test_bow_vector_large_then_small(ex, delay_ex, cases):
    """n_max = 5000 asks for more than the default LDS (hipFuncSetAttribute on the host, no wait), 300 does not; back to back"""
    run_and_check(delay_ex, lambda: [step(cases["bow_vector", "n_max 5000"], ex), step(cases["bow_vector", "n_max 300"], ex)], "bow vector 5000, 300")


def test_records_bow_match_grow_then_smaller(ex, delay_ex, cases):
    """world 5, cap 301 on a vocabulary whose scratch is empty: it grows (the library drains the device: stated), then world 5, cap 64 in the same
    scratch without a wait"""
    from hyslam_amd import _native as N
    from hyslam_amd import distributed as D
    import scenes
    e = S.vocab_tree()
    made = []

    def scene():
        voc = D.DeviceVocabulary(ex, scenes.tree_struct(N.VocabTree, e["tree"]), S.LEVELSUP, keepalive=e["tree"])
        made.append(voc)
        return [step(cases["records_bow_match", "set 5"], ex, voc=voc, waits="the vocabulary's scratch grows"), step(cases["records_bow_match", "set 4"], ex, voc=voc)]
    run_and_check(delay_ex, scene, "records bow match")
    for v in made:
        v.close()


# ---------------------------------------------------------------- place recognition
def place_db(HS, ex, sc):
    db = HS.PlaceRecognizer(sc["n_words"], ex)
    for i, (key, w, v) in enumerate(sc["host"]):                  # the host form: returns when the copy is done; the storage is allocated here
        assert db.add(key, (w, v)) == i
    return db


def test_place_add_then_queries(HS, ex, delay_ex):
    """two hs_place_db_add_device, then hs_place_query_reloc_device (the first query after an add: waits for the stream and uploads the walk order)
    and hs_place_query_loop_device (steady state: waits for nothing).  The adds have no output: the queries show whether the vectors had arrived"""
    sc = S.place_scene()
    made = []

    def scene():
        db = place_db(HS, ex, sc)
        made.append(db)
        waits = [None, None, "the first query after an add uploads the walk order", None]
        return [step(c, ex, db=db, waits=w) for c, w in zip(sc["steps"], waits)]
    run_and_check(delay_ex, scene, "place add, add, reloc, loop")
    for db in made:
        db.close()


def test_mixed_chain_on_one_stream(HS, delay_ex, vocabulary, ex):
    """extract -> BoW transform -> BoW vector -> place add -> place query: every stage reads what the stage before it left on the device; the image
    arrives late, nothing is waited for between the calls but inside the query (the first after an add)"""
    ex.reserve(S.W, S.H, 1)
    cap = ex.max_keypoints()
    sc = S.chain_scene(cap)
    made = []

    def scene():
        db = place_db(HS, ex, sc)
        made.append(db)
        waits = [None, None, None, None, "the first query after an add uploads the walk order"]
        return [step(c, ex, voc=vocabulary, db=db, waits=w) for c, w in zip(sc["steps"], waits)]
    st, s0 = step(sc["steps"][0], ex), hipmem.Stream()              # the handle has extracted at this size before: nothing is configured under the delay
    bufs = {k: hipmem.DevBuf.from_numpy(SO._raw(d)) for k, (r, d) in sc["steps"][0].inputs.items()}
    bufs.update({k: hipmem.DevBuf(n) for k, n in sc["steps"][0].outputs.items()})
    st.call({k: b.ptr for k, b in bufs.items()}, s0.ptr)
    s0.synchronize()
    run_and_check(delay_ex, scene, "mixed chain")
    for db in made:
        db.close()


# ---------------------------------------------------------------- the negative control
def test_the_harness_sees_a_call_on_another_stream(HS, delay_ex, cases):
    """the harness has teeth: the same sequence, but the TEST hands hs_landmark_best_descriptors_device a second stream while the inputs arrive late on
    s (and waits for that second stream, so that the outcome does not hang on how two queues interleave).  The snapshot taken on s must differ from the
    reference: it holds the decoy's result or 0x55.  The decoy is a valid case: nothing reads out of range, nothing is provoked"""
    own = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=500), device=0)
    other = hipmem.Stream(non_blocking=True)
    c = cases["landmark_best_descriptors", "large"]

    def scene():
        st = step(c, own)
        inner = st.call

        def call(p, s):
            inner(p, s)
            hipmem._ok(hipmem.hip().hipStreamSynchronize(s), "hipStreamSynchronize")
        st.call = call
        return [st]
    for steps, got, after in SO.run(delay_ex, scene, call_stream=other, tag="negative control"):
        bad = SO.mismatches(steps[0], got[0])
        print("negative control:", bad)
        assert {k for k, _, _ in bad} == {"best", "median"}, "a call on another stream went unnoticed"
        assert all(what in ("the decoy's result", "0x55") for _, _, what in bad), bad
    own.close()
