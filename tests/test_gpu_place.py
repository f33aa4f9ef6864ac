"""GPU: hs_bow_vector, hs_place_db_* and hs_place_query_* — PlaceRecognizer (src/core/PlaceRecognizer.cpp:43-311) on DBoW2's L1 score — bit for bit
against the restatement in tests/ref_place.py (pinned by tests/test_place_ref.py): candidates, per-slot counts, scores and accumulations (compared
as raw float bit patterns) and pBestKF, through the Python classes, the host-pointer and the device-pointer entry points."""
import ctypes as C

import numpy as np
import pytest

import hipmem
import ref_place as R
from place_cases import BOW_LAST_BIT, KNOWN, N_WORDS, SCENES, random_scene, ref_query, run_ref, scene_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex(gpu):
    import hyslam_amd as HS
    return HS.ORBExtractor(device=0)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def per_slot(rec, det):
    """the restatement's dicts by key -> the library's per-slot arrays"""
    n = len(rec._keys)
    words, score, acc, best = np.full(n, -1, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.full(n, -1, np.int32)
    for k, s in rec._slot.items():
        if k in det["words"]:
            words[s], score[s] = det["words"][k], det["score"][k]
        if k in det["best"]:
            acc[s], best[s] = det["acc"][k], rec._slot[det["best"][k]]
    return dict(words=words, score=score, acc=acc, best=best)


def assert_query(rec, got_keys, got, want_keys, det, tag=""):
    assert got_keys == want_keys, (tag, got_keys[:8], want_keys[:8])
    want = per_slot(rec, det)
    for k in ("words", "best"):
        bad = np.nonzero(got[k] != want[k])[0]
        assert not len(bad), (tag, k, bad[:5], got[k][bad[:5]], want[k][bad[:5]])
    for k in ("score", "acc"):
        bad = np.nonzero(bits(got[k]) != bits(want[k]))[0]
        assert not len(bad), (tag, k, bad[:5], got[k][bad[:5]], want[k][bad[:5]])


def fill(HS, ex, n_words, entries, erased):
    rec = HS.PlaceRecognizer(n_words, ex)
    for key, w, v in entries:
        rec.add(key, (w, v))
    for key in erased:
        rec.erase(key)
    return rec


def gpu_query(rec, q, neigh):
    if q["mode"] == "reloc":
        return rec.detectRelocalizationCandidates(q["query"], neigh, details=True)
    return rec.detectLoopCandidates(q["query"], q["min_score"], q["connected"], neigh, details=True)


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_case(ex, name):
    import hyslam_amd as HS
    case = KNOWN[name]
    rec = fill(HS, ex, N_WORDS, case["entries"], case["erased"])
    keys, got = gpu_query(rec, case, case["neigh"])
    assert keys == case["expect"]                                       # the hand-derived answer itself
    want_keys, det, _ = run_ref(R, case)
    assert_query(rec, keys, got, want_keys, det, name)
    for k, v in case.get("score", {}).items():
        assert bits(got["score"][rec._slot[k]]) == bits(v), (name, k)


@pytest.mark.parametrize("scene", SCENES, ids=lambda s: "%dkf_%dwords" % (s[1], s[2]))
def test_seeded_scene(ex, scene):
    import hyslam_amd as HS
    seed, n_kf, n_words, lens, big, n_queries = scene
    sc = random_scene(seed, n_kf, n_words, lens, big, n_queries)
    rec = fill(HS, ex, n_words, sc["entries"], sc["erased"])
    assert rec.size() == (n_kf - len(sc["erased"]), n_kf)
    ref = scene_ref(R, sc)
    multi = 0
    for i, q in enumerate(sc["queries"]):
        want_keys, det = ref_query(ref, sc, q)
        keys, got = gpu_query(rec, q, sc["neigh"])
        assert_query(rec, keys, got, want_keys, det, (seed, i, q["mode"]))
        multi += len(keys) >= 2
    if n_kf == 500:
        assert 2 * multi >= len(sc["queries"])                          # the scenes do exercise the select pass
        for branch in ("replace", "dedupe", "excluded", "d9", "tombstone"):
            assert ref.trace[branch] > 0, branch
    rec.close()


def test_no_shared_word_is_an_empty_result(ex):
    import hyslam_amd as HS
    sc = random_scene(3, 200, 1000, (5, 30))
    rec = fill(HS, ex, 2000, sc["entries"], [])
    q = (np.arange(1000, 1040, dtype=np.int32), np.full(40, 1 / 40))
    keys, got = rec.detectRelocalizationCandidates(q, sc["neigh"], details=True)
    assert keys == [] and (got["words"] == -1).all() and (got["best"] == -1).all() and not got["score"].any()
    assert rec.detectLoopCandidates(q, 0.0, [], sc["neigh"]) == []
    assert rec.detectRelocalizationCandidates(({}), sc["neigh"]) == []   # an empty query vector


def test_long_query_vectors(ex):
    """queries of thousands of words (many blocks of the scatter pass): the 10 000-word stored vector itself, and 5 000 words of it"""
    import hyslam_amd as HS
    seed, n_kf, n_words, lens, big, _ = SCENES[3]
    sc = random_scene(seed, n_kf, n_words, lens, big, 1)
    rec = fill(HS, ex, n_words, sc["entries"], sc["erased"])
    ref = scene_ref(R, sc)
    long_kf = next(e for e in sc["entries"] if len(e[1]) == 10000)
    assert long_kf[0] not in sc["erased"]
    for n, mode in ((10000, "reloc"), (10000, "loop"), (5000, "reloc"), (257, "loop")):
        q = dict(mode=mode, query=(long_kf[1][:n], long_kf[2][:n] / long_kf[2][:n].sum()), connected=[], min_score=0.0)
        keys, got = gpu_query(rec, q, sc["neigh"])
        want_keys, det = ref_query(ref, sc, q)
        assert_query(rec, keys, got, want_keys, det, (n, mode))
        assert long_kf[0] in keys and got["words"][rec._slot[long_kf[0]]] == n - (mode == "loop")


def test_every_slot_a_tombstone(ex):
    """slots > 0 and nothing live: no candidate, and the per-slot arrays say -1 / 0, not what the previous query left"""
    import hyslam_amd as HS
    rec = fill(HS, ex, N_WORDS, KNOWN["replace_dedupe_reloc"]["entries"], [])
    keys, got = rec.detectRelocalizationCandidates(KNOWN["replace_dedupe_reloc"]["query"], None, details=True)
    assert len(keys) == 3 and (got["words"] > 0).all()
    for k in (10, 20, 40):
        rec.erase(k)
    assert rec.size() == (0, 3)
    for loop in (False, True):
        keys, got = rec._query(loop, KNOWN["replace_dedupe_reloc"]["query"], None, (), 0.0, True)
        assert keys == [] and (got["words"] == -1).all() and (got["best"] == -1).all() and not got["score"].any() and not got["acc"].any()


def test_erase_query_add_again_clear_and_reuse(ex):
    import hyslam_amd as HS
    sc = random_scene(21, 300, 1000, (5, 60), n_queries=4)
    rec = fill(HS, ex, 1000, sc["entries"], sc["erased"])
    ref = scene_ref(R, sc)
    gone = [e[0] for e in sc["entries"] if e[0] not in sc["erased"]][10:40:3]
    for k in gone:
        rec.erase(k)
        ref.erase(k)
    for i, q in enumerate(sc["queries"]):
        keys, got = gpu_query(rec, q, sc["neigh"])
        want_keys, det = ref_query(ref, sc, q)
        assert_query(rec, keys, got, want_keys, det, ("erased", i))
    back = {e[0]: e for e in sc["entries"]}
    for k in gone[:5]:                                                   # the same keys come back in NEW slots
        s = rec.add(k, back[k][1:])
        assert s >= 300
        ref.add(*back[k])
    for i, q in enumerate(sc["queries"]):
        keys, got = gpu_query(rec, q, sc["neigh"])
        want_keys, det = ref_query(ref, sc, q)
        assert_query(rec, keys, got, want_keys, det, ("added again", i))
    assert ex._lib.hs_place_db_erase(rec._db, 10 ** 6) == 1
    for n_kf, seed in ((40, 22), (1500, 23), (3, 24)):                   # clear keeps the allocations; the handle serves other sizes
        rec.clear()
        assert rec.size() == (0, 0)
        sc = random_scene(seed, n_kf, 1000, (5, 60), n_queries=2)
        for key, w, v in sc["entries"]:
            rec.add(key, (w, v))
        ref = scene_ref(R, dict(sc, erased=[]))
        for i, q in enumerate(sc["queries"]):
            keys, got = gpu_query(rec, q, sc["neigh"])
            want_keys, det = ref_query(ref, sc, q)
            assert_query(rec, keys, got, want_keys, det, ("cleared", n_kf, i))


def test_refusals_and_capacity(ex):
    from hyslam_amd import _native as N
    L = ex._lib
    db = C.c_void_p()
    assert L.hs_place_db_create(ex._h, 1000, 1, C.byref(db)) == N.HS_ERR_INVALID        # L2_NORM: not implemented
    assert L.hs_place_db_create(ex._h, 0, 0, C.byref(db)) == N.HS_ERR_INVALID
    assert L.hs_place_db_create(ex._h, 1000, 0, C.byref(db)) == N.HS_OK
    slot = C.c_int32()
    w, v = np.array([1, 2, 3], np.int32), np.array([0.5, 0.25, 0.25])
    for bw, bv in ((np.array([2, 1, 3], np.int32), v), (np.array([1, 1, 3], np.int32), v), (np.array([1, 2, 1000], np.int32), v),
                   (w, np.array([0.5, 0.0, 0.5])), (w, np.array([0.5, np.inf, 0.5])), (w, np.array([0.5, np.nan, 0.5])), (w, np.array([0.5, -0.25, 0.5]))):
        assert L.hs_place_db_add(db, 1, p(bw), p(bv), 3, C.byref(slot)) == N.HS_ERR_INVALID
    for key in (30, 10, 20):
        assert L.hs_place_db_add(db, key, p(w), p(v), 3, C.byref(slot)) == N.HS_OK
    cand, n = np.full(3, -7, np.int32), C.c_int32()
    assert L.hs_place_query_reloc(db, p(w), p(v), 3, None, p(cand), 2, C.byref(n), None, None, None, None) == N.HS_ERR_CAPACITY
    assert n.value == 3 and (cand == -7).all()                                          # nothing partial
    assert L.hs_place_query_reloc(db, p(w), p(v), 3, None, p(cand), 3, C.byref(n), None, None, None, None) == N.HS_OK
    assert n.value == 3 and cand.tolist() == [1, 2, 0]                                  # ascending key: 10, 20, 30
    # the device form: the count always, no candidate when it exceeds cap
    d_w, d_v = hipmem.DevBuf.from_numpy(w), hipmem.DevBuf.from_numpy(v)
    d_c, d_n = hipmem.DevBuf(16), hipmem.DevBuf(4)
    d_c.fill(0x55)
    assert L.hs_place_query_reloc_device(db, d_w.ptr, d_v.ptr, None, 3, None, d_c.ptr, 2, d_n.ptr, None, None, None, None, None) == N.HS_OK
    ex.synchronize()
    assert d_n.to_numpy(np.int32, 1)[0] == 3 and (d_c.to_numpy(np.uint32, 3) == 0x55555555).all()
    L.hs_place_db_destroy(db)


def test_bow_vector_against_containers(ex):
    import hyslam_amd as HS
    voc = HS.ORBVocabulary.__new__(HS.ORBVocabulary)
    voc._vocab, voc._ex = None, ex
    c = BOW_LAST_BIT
    w, v = voc.bow_vector(c["word"], np.float32(c["weight"]))
    assert (w.tolist(), v.tolist()) == c["expect"]
    rng = np.random.default_rng(7)
    for n, n_words in ((0, 10), (1, 10), (63, 50), (64, 5), (65, 1000), (1000, 300), (1024, 100000), (1025, 40), (2500, 1000000), (8192, 3), (16384, 5000)):
        word = rng.integers(0, n_words, n).astype(np.int32)
        weight = (rng.random(n) * 10 ** rng.uniform(-3, 3, n)).astype(np.float32)
        weight[rng.random(n) < 0.1] = 0.0
        w, v = voc.bow_vector(word, weight)
        bow = HS.ORBVocabulary.containers(word, weight, np.zeros(n, np.int32))[0]
        rw, rv = R.bow_vector(word, weight)
        assert w.tolist() == rw == sorted(bow) and v.view(np.uint64).tolist() == np.array(rv, np.float64).view(np.uint64).tolist(), n
        assert v.tolist() == [bow[k] for k in sorted(bow)], n
    assert ex._lib.hs_bow_vector(ex._h, p(word), p(weight), 16385, p(w), p(v), C.byref(C.c_int32())) == 1


def test_vocabulary_score(ex):
    import hyslam_amd as HS
    voc = HS.ORBVocabulary.__new__(HS.ORBVocabulary)
    voc._vocab, voc._ex, voc.size = None, ex, lambda: 1000
    a = {1: 0.5, 2: 0.5}
    assert voc.score(a, a) == 1.0 and voc.score(a, {2: 0.25, 3: 0.75}) == 0.25 and voc.score(a, {7: 1.0}) == 0.0
    rng = np.random.default_rng(9)
    for _ in range(20):
        va = {int(k): float(x) for k, x in zip(rng.choice(1000, 70, replace=False), rng.random(70) + 0.01)}
        vb = {int(k): float(x) for k, x in zip(rng.choice(1000, 300, replace=False), rng.random(300) + 0.01)}
        assert bits(voc.score(va, vb)) == bits(np.float32(R.l1_score(sorted(va.items()), sorted(vb.items()))))


def test_device_chain_equals_host_path(ex):
    """hs_bow_transform_device -> hs_bow_vector_device -> hs_place_db_add_device / hs_place_query_*_device on ONE stream, nothing read by the host in
    between; the result equals the host-pointer path on the same descriptors"""
    import hyslam_amd as HS
    import oracle
    from hyslam_amd import _native as N
    L = ex._lib
    tree, keep, n_words = oracle.make_vocab_tree(N.VocabTree, 6, 3, 5)
    voc = HS.ORBVocabulary(tree, ex)
    assert voc.size() == n_words
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (int(rng.integers(200, 900)), 32), dtype=np.uint8) for _ in range(12)]
    frames += [f ^ (rng.random(f.shape) < 0.02).astype(np.uint8) for f in frames[:4]]       # near copies: they share most words
    # host path
    host = HS.PlaceRecognizer(n_words, ex)
    vecs = []
    for i, d in enumerate(frames):
        _, _, (word, weight, _) = voc.transform(d)
        vecs.append(voc.bow_vector(word, weight))
        host.add(100 - i, vecs[-1])
    neigh = {100 - i: [100 - j for j in range(len(frames)) if j != i][:10] for i in range(len(frames))}
    want = [host.detectRelocalizationCandidates(vecs[k], neigh, details=True) for k in (0, 13)]
    want_loop = host.detectLoopCandidates(vecs[1], 0.01, [100 - 1], neigh, details=True)
    # device path
    vd = C.c_void_p()
    N.check(ex._h, L.hs_vocab_upload(ex._h, C.byref(tree), 4, C.byref(vd)))
    s = hipmem.Stream()
    dev = HS.PlaceRecognizer(n_words, ex)
    cap = 1024
    bufs = []
    for i, d in enumerate(frames):
        dd, dn = hipmem.DevBuf.from_numpy(d), hipmem.DevBuf.from_numpy(np.array([len(d)], np.int32))
        o = [hipmem.DevBuf(cap * 4) for _ in range(4)] + [hipmem.DevBuf(cap * 8), hipmem.DevBuf(4)]   # word, weight, node, bow word, bow value, m
        N.check(ex._h, L.hs_bow_transform_device(ex._h, vd, dd.ptr, dn.ptr, cap, o[0].ptr, o[1].ptr, o[2].ptr, s.ptr))
        N.check(ex._h, L.hs_bow_vector_device(ex._h, o[0].ptr, o[1].ptr, dn.ptr, cap, o[3].ptr, o[4].ptr, o[5].ptr, s.ptr))
        dev.add_device(100 - i, o[3].ptr, o[4].ptr, o[5].ptr, cap, s.ptr)
        bufs.append((dd, dn, o))
    slots = len(frames)
    d_neigh = hipmem.DevBuf.from_numpy(dev.neighbour_table(neigh))
    excl = np.zeros(slots, np.uint8); excl[dev._slot[99]] = 1
    d_excl = hipmem.DevBuf.from_numpy(excl)
    outs = []
    for k, loop in ((0, 0), (13, 0), (1, 1)):
        o = bufs[k][2]
        r = [hipmem.DevBuf(slots * 4) for _ in range(5)] + [hipmem.DevBuf(4)]                  # cand, words, score, acc, best, n
        if loop:
            st = L.hs_place_query_loop_device(dev._db, o[3].ptr, o[4].ptr, o[5].ptr, cap, d_excl.ptr, 0.01, d_neigh.ptr, r[0].ptr, slots, r[5].ptr,
                                              r[1].ptr, r[2].ptr, r[3].ptr, r[4].ptr, s.ptr)
        else:
            st = L.hs_place_query_reloc_device(dev._db, o[3].ptr, o[4].ptr, o[5].ptr, cap, d_neigh.ptr, r[0].ptr, slots, r[5].ptr,
                                               r[1].ptr, r[2].ptr, r[3].ptr, r[4].ptr, s.ptr)
        N.check(ex._h, st)
        outs.append(r)
    s.synchronize()
    for r, (wkeys, wdet) in zip(outs, want + [want_loop]):
        n = int(r[5].to_numpy(np.int32, 1)[0])
        assert [dev._keys[x] for x in r[0].to_numpy(np.int32, n)] == wkeys and len(wkeys) >= 1
        assert np.array_equal(r[1].to_numpy(np.int32, slots), wdet["words"]) and np.array_equal(r[4].to_numpy(np.int32, slots), wdet["best"])
        assert np.array_equal(bits(r[2].to_numpy(np.float32, slots)), bits(wdet["score"]))
        assert np.array_equal(bits(r[3].to_numpy(np.float32, slots)), bits(wdet["acc"]))
    L.hs_vocab_dev_destroy(vd)


def test_cpp_adaptor(tmp_path):
    """hyslam_amd/host/HipPlaceRecognizer.h through tests/cpp/test_place_adaptor.cpp: the same scene, the same candidates"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build = os.path.join(root, "tests", "cpp", "_build")
    exe = os.path.join(build, "test_place_adaptor")
    os.makedirs(build, exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(root, "tests", "cpp", "test_place_adaptor.cpp"),
                           "-o", exe, "-L" + os.path.join(root, "hyslam_amd"), "-lhyslam_amd", "-Wl,-rpath," + os.path.join(root, "hyslam_amd")])
    sc = random_scene(31, 400, 1000, (5, 60), n_queries=8)
    i32, u64 = (lambda x: np.int32(x).tobytes()), (lambda x: np.asarray(x, np.uint64).tobytes())
    vecb = lambda w, v: i32(len(w)) + np.asarray(w, np.int32).tobytes() + np.asarray(v, np.float64).tobytes()
    blob = i32(1000) + i32(len(sc["entries"]))
    for key, w, v in sc["entries"]:
        nb = sc["neigh"][key]
        blob += u64(key) + vecb(w, v) + i32(len(nb)) + u64(nb)
    blob += i32(len(sc["erased"])) + u64(sc["erased"]) + i32(len(sc["queries"]))
    for q in sc["queries"]:
        blob += i32(q["mode"] == "loop") + np.float32(q["min_score"]).tobytes() + vecb(*q["query"]) + i32(len(q["connected"])) + u64(q["connected"])
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"PLACE ADAPTOR OK" in r.stdout, r.stdout + r.stderr
    raw = (tmp_path / "out.bin").read_bytes()
    ref = scene_ref(R, sc)
    off = 0
    for q in sc["queries"]:
        n = int(np.frombuffer(raw, np.int32, 1, off)[0])
        got = np.frombuffer(raw, np.uint64, n, off + 4).tolist()
        off += 4 + 8 * n
        assert got == ref_query(ref, sc, q)[0]
    assert off == len(raw)


def test_end_to_end_true_neighbours_are_candidates(ex):
    """Frames -> extractor -> vocabulary transform -> BoW vector -> place query, on rendered images.  Two rigs of 8 cameras (hyslam_amd/synth.py:
    camera i sees columns [i * w/4, i * w/4 + w) of its rig's panorama, so cameras i and i +- 1 share three quarters of their view; the two rigs look
    at different scenes).  The query is one camera of rig A, the database every other frame of both rigs.  Ground truth is the geometry: the query's
    adjacent cameras must be candidates, the best-scoring key frame must be one of them, and each of them must outscore every frame of the other
    rig.  Through the host-pointer calls and through the device chain (extract_batch_device -> hs_bow_transform_device -> hs_bow_vector_device ->
    hs_place_db_add_device / hs_place_query_*_device on one stream); both must also equal the restatement."""
    import hyslam_amd as HS
    from hyslam_amd import _native as N, synth
    from place_cases import trained_vocab_tree
    L = ex._lib
    W, H, CAMS = 640, 480, 8
    train = np.concatenate([ex(synth.synth_image(900 + i, W, H))[1] for i in range(6)])
    tree, keep, n_words = trained_vocab_tree(N.VocabTree, train, 10, 4, 5)
    voc = HS.ORBVocabulary(tree, ex)
    frames = [("A", i, im) for i, im in enumerate(synth.synth_rig(101, CAMS, W, H))] + [("B", i, im) for i, im in enumerate(synth.synth_rig(202, CAMS, W, H))]
    vecs = []
    for _, _, im in frames:
        _, d = ex(im)
        _, _, (word, weight, _) = voc.transform(d)
        vecs.append(voc.bow_vector(word, weight))
    key_of = lambda j: 1000 + (j * 37) % 101                              # key order unrelated to the cameras
    for qcam in (3, 0, 7):
        db = [j for j in range(len(frames)) if j != qcam]
        adjacent = {key_of(j) for j in db if frames[j][0] == "A" and abs(frames[j][1] - qcam) == 1}
        other_rig = [key_of(j) for j in db if frames[j][0] == "B"]
        neigh = {key_of(j): [key_of(k) for k in db if frames[k][0] == frames[j][0] and abs(frames[k][1] - frames[j][1]) == 1] for j in db}
        host, ref = HS.PlaceRecognizer(n_words, ex), R.PlaceRecognizerRef(n_words)
        for j in db:
            host.add(key_of(j), vecs[j])
            ref.add(key_of(j), *vecs[j])
        q = vecs[qcam]
        # no covisibility: every retained key frame stands for itself
        keys, got = host.detectRelocalizationCandidates(q, None, details=True)
        want_keys, det = ref.detect_reloc(q[0], q[1], {})
        assert_query(host, keys, got, want_keys, det, ("e2e reloc", qcam))
        score = {k: float(got["score"][s]) for k, s in host._slot.items()}
        assert adjacent <= set(keys), (qcam, adjacent, keys)
        assert max(score, key=score.get) in adjacent, (qcam, score)
        assert min(score[k] for k in adjacent) > max(score[k] for k in other_rig), (qcam, score)
        lkeys, lgot = host.detectLoopCandidates(q, 0.05, [], None, details=True)
        assert adjacent <= set(lkeys) and lkeys == ref.detect_loop(q[0], q[1], [], 0.05, {})[0]
        # with covisibility (adjacent cameras of a rig): equal to the restatement, and the candidates still name the query's side of rig A
        ckeys, cgot = host.detectRelocalizationCandidates(q, neigh, details=True)
        want_keys, det = ref.detect_reloc(q[0], q[1], neigh)
        assert_query(host, ckeys, cgot, want_keys, det, ("e2e covisible", qcam))
        assert set(ckeys) & adjacent, (qcam, ckeys)
        host.close()
    # the device chain for the last query camera
    qcam = 7
    db = [j for j in range(len(frames)) if j != qcam]
    cap = ex.max_keypoints()
    assert cap <= 16384
    s = hipmem.Stream()
    imgs = np.ascontiguousarray(np.stack([f[2] for f in frames]))
    nf = len(frames)
    d_img = hipmem.DevBuf.from_numpy(imgs)
    d_kps, d_desc, d_n = hipmem.DevBuf(nf * cap * N.KP_DTYPE.itemsize), hipmem.DevBuf(nf * cap * 32), hipmem.DevBuf(nf * 4)
    ex.extract_batch_device(d_img.ptr, nf, W, H, W, W * H, d_kps.ptr, d_desc.ptr, d_n.ptr, cap, s.ptr)
    vd = C.c_void_p()
    N.check(ex._h, L.hs_vocab_upload(ex._h, C.byref(tree), 4, C.byref(vd)))
    dev = HS.PlaceRecognizer(n_words, ex)
    bow = []
    for j in range(nf):
        o = [hipmem.DevBuf(cap * 4) for _ in range(4)] + [hipmem.DevBuf(cap * 8), hipmem.DevBuf(4)]       # word, weight, node, bow word, bow value, m
        N.check(ex._h, L.hs_bow_transform_device(ex._h, vd, d_desc.ptr + j * cap * 32, d_n.ptr + 4 * j, cap, o[0].ptr, o[1].ptr, o[2].ptr, s.ptr))
        N.check(ex._h, L.hs_bow_vector_device(ex._h, o[0].ptr, o[1].ptr, d_n.ptr + 4 * j, cap, o[3].ptr, o[4].ptr, o[5].ptr, s.ptr))
        if j != qcam:
            dev.add_device(key_of(j), o[3].ptr, o[4].ptr, o[5].ptr, cap, s.ptr)
        bow.append(o)
    slots = len(db)
    r = [hipmem.DevBuf(slots * 4) for _ in range(5)] + [hipmem.DevBuf(4)]                                 # cand, words, score, acc, best, n
    o = bow[qcam]
    N.check(ex._h, L.hs_place_query_reloc_device(dev._db, o[3].ptr, o[4].ptr, o[5].ptr, cap, None, r[0].ptr, slots, r[5].ptr,
                                                 r[1].ptr, r[2].ptr, r[3].ptr, r[4].ptr, s.ptr))
    s.synchronize()
    n = int(r[5].to_numpy(np.int32, 1)[0])
    assert [dev._keys[x] for x in r[0].to_numpy(np.int32, n)] == keys                                     # the host path's answer for camera 7
    assert np.array_equal(r[1].to_numpy(np.int32, slots), got["words"]) and np.array_equal(bits(r[2].to_numpy(np.float32, slots)), bits(got["score"]))
    assert {key_of(j) for j in db if frames[j][0] == "A" and frames[j][1] == 6} <= set(dev._keys[x] for x in r[0].to_numpy(np.int32, n))
    L.hs_vocab_dev_destroy(vd)
