"""GPU: no result may depend on what the library's own device memory held before the call (hs_debug_poison, include/hyslam_amd.h).

Every host-pointer entry point lays its pieces out in the handle's grow-only scratch arena (HsStage, hs_internal.h) and copies its `out` pieces back in
full, so an element a kernel never wrote, or a temporary it read before writing, comes back as whatever the arena held — zeros in a fresh process, the
previous call's data in a long-lived handle.  Here each entry point runs with the arena (and, in the last group, every device allocation the library
makes for itself) filled with 0x00 (what a fresh process sees), 0xFF (int -1, the library's own "none"; NaN; every flag set) and 0xA5 (a large
negative int, a non-zero flag that is not 1), and

  (a) every result equals the reference the entry point's own test module uses (the oracle, or the ref_* restatement on the *_cases.py builders),
  (b) the results under the three bytes are byte-identical to each other,
  (c) the violation counter does not move: no kernel stored into the padding between two staged pieces or into the slack behind the last one,
  (d) the host outputs go in filled with a fourth value (0x3C, or the sentinel of the helper that is reused), so that an element the call leaves
      alone is told apart from one that came back from the arena.

Sizes are 0 (where the entry point accepts it), 1, 65 and 300, CSR inputs with an empty first, middle and last row, `cap` below, at and above the
produced count, and each sequence starts at 300 and goes on at 1 on the same handle, so the large arena is reused under poison.  The helpers of the
entry points' own test modules are imported, no reference is written here.  The module switches poisoning off again when it is done."""
import ctypes as C
import functools

import numpy as np
import pytest

import hipmem
import oracle
import poseopt_cases as P
import ref_kfgraph as RK
import ref_landmark_entry as RLE
import ref_localmap as RL
import ref_place as RP
import scenes
import test_gpu_area_edges as AE
import test_gpu_bow_edges as BE
import test_gpu_kfgraph as KG
import test_gpu_landmark_descriptors as LD
import test_gpu_landmark_entries as LE
import test_gpu_place as PL
import test_gpu_poseopt as PO
import hyslam_amd as HS
from hyslam_amd import _native as N
from hyslam_amd.distributed import DeviceVocabulary
from hyslam_amd.synth import synth_image, synth_stereo_pair
from kfgraph_cases import csr, random_candidates, random_table, table
from landmark_entry_cases import random_batch
from localmap_cases import random_keyframes, random_points
from place_cases import random_scene, ref_query, scene_ref
from ref_landmark import distinctive_descriptors_fast

pytestmark = pytest.mark.gpu
f32 = np.float32
BYTES = (0x00, 0xFF, 0xA5)
SENT = 0x3C


@pytest.fixture(scope="module")
def lib(gpu):
    L = N.lib()
    yield L
    L.hs_debug_poison(-1)                              # no later module of the same process runs poisoned


@pytest.fixture(scope="module")
def matcher(lib):
    return HS.FeatureMatcher(HS.FeatureMatcherSettings(nnratio=0.8), HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=500)))


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def sentinel(shape, dtype):
    a = np.empty(shape, dtype)
    a.reshape(-1).view(np.uint8)[:] = SENT
    return a


def raw(x):
    return np.ascontiguousarray(x).tobytes()


def same_bits(g, w):
    g, w = np.asarray(g), np.asarray(w)
    if g.shape != w.shape:
        return False
    if g.dtype.kind == "f":
        return g.dtype == w.dtype and raw(g) == raw(w)
    return bool(np.array_equal(g, w))


def exact(*want):
    """(a), bit for bit: every output against the reference's"""
    def check(out):
        assert len(out) == len(want)
        for i, (g, w) in enumerate(zip(out, want)):
            assert same_bits(g, w), "output %d differs from the reference: got %s want %s" % (i, np.asarray(g).reshape(-1)[:8], np.asarray(w).reshape(-1)[:8])
    return check


def under_poison(lib, cases):
    """cases: (tag, run, check) in call order; run() -> the outputs of one call, check(outputs) asserts (a).  Runs the whole sequence under every byte
    of BYTES, then asserts (b) and (c)."""
    before = lib.hs_debug_poison_violations()
    seen = {}
    try:
        for byte in BYTES:
            assert lib.hs_debug_poison(byte) == N.HS_OK
            for i, (tag, run, check) in enumerate(cases):
                out = run()
                try:
                    check(out)
                except AssertionError as e:
                    raise AssertionError("%s under poison 0x%02X: %s" % (tag, byte, e)) from None
                seen.setdefault((i, tag), []).append(tuple(raw(o) for o in out))
    finally:
        lib.hs_debug_poison(-1)
    for (i, tag), outs in seen.items():
        assert outs[0] == outs[1], "%s: the outputs under 0x00 and 0xFF differ" % (tag,)
        assert outs[0] == outs[2], "%s: the outputs under 0x00 and 0xA5 differ" % (tag,)
    assert lib.hs_debug_poison_violations() == before, "a kernel stored outside its staged piece"
    assert len(seen) == len(cases) > 0


# ---------------------------------------------------------------- grid-area matchers (tests/scenes.py area cases, the oracle)
AREA_SIZES = ((300, 300, "mixed"), (1, 1, "mixed"), (65, 65, "ties"), (0, 5, "mixed"), (300, 65, "radius"), (65, 300, "landmark_edges"), (1, 0, "bounds"))


@functools.lru_cache(None)
def area_cases():
    rng = np.random.default_rng(4242)
    out = []
    for n, L, kind in AREA_SIZES:
        c = scenes._area_case(rng, kind, n=n, L=L)
        c["sim3"] = scenes.area_sim3_pair(rng, c)
        c["Fo"], c["_ko"] = oracle.make_frame_view(oracle.FrameView, **c["fa"])
        c["Fg"], c["_kg"] = oracle.make_frame_view(N.FrameView, **c["fa"])
        c["tag"] = (kind, len(c["fa"]["kps"]), len(c["lms"]))
        out.append(c)
    return out


def native_pp(pp):
    return N.ProjParams(*[getattr(pp, k) for k, _ in oracle.ProjParams._fields_])


def c_projection(m, Fg, lms, pp, token=None):
    """hs_search_by_projection / hs_search_by_projection_frame through the C ABI on sentinel-filled outputs"""
    ex = m._ex
    lms = np.ascontiguousarray(lms, N.LM_DTYPE)
    L = len(lms)
    midx, mdist, n = sentinel(L, np.int32), sentinel(L, f32), C.c_int32(SENT)
    pn = native_pp(pp)
    if token is None:
        st = ex._lib.hs_search_by_projection(ex._h, C.byref(Fg), p(lms), L, C.byref(pn), p(midx), p(mdist), C.byref(n))
    else:
        st = ex._lib.hs_search_by_projection_frame(ex._h, C.c_uint64(token), C.byref(Fg), p(lms), L, C.byref(pn), p(midx), p(mdist), C.byref(n))
    N.check(ex._h, st)
    return midx, mdist, n.value


@pytest.mark.parametrize("preset", ["local map", "last frame", "fuse"], ids=["plain", "check_rotation", "first_wins"])
def test_search_by_projection(lib, matcher, preset):
    """the plain criterion; check_rotation (d_pangle, d_winner through k_rotation_filter); first_wins (Fuse: d_winner through k_first_wins)"""
    cases = []
    for c in area_cases():
        pp = next(x[2] for x in AE.presets(matcher, float(c["th"])) if x[0] == preset)
        if len(c["lms"]) == 0:
            want = (np.zeros(0, np.int32), np.zeros(0, f32), 0)
        else:
            want = oracle.search_by_projection(c["Fo"], c["lms"], pp)
        cases.append((c["tag"], functools.partial(c_projection, matcher, c["Fg"], c["lms"], pp), exact(*want)))
    under_poison(lib, cases)


def c_projection_device(m, fa, lms, pp, posed):
    """hs_search_by_projection_device / _posed_device: frame arrays, landmarks and pose in device memory, on a caller stream"""
    ex = m._ex
    Fg, keep = oracle.make_frame_view(N.FrameView, **fa)
    bufs = [hipmem.DevBuf.from_numpy(np.ascontiguousarray(a)) for a in (fa["kps"], fa["desc"], fa["uR"], fa["kp_lm_obs"], lms)]
    Fg.kps, Fg.desc, Fg.uR, Fg.kp_lm_obs = bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr
    L = len(lms)
    d_i, d_d, d_n = hipmem.DevBuf(L * 4, zero=False), hipmem.DevBuf(L * 4, zero=False), hipmem.DevBuf(4, zero=False)
    for b in (d_i, d_d, d_n):
        b.fill(SENT)
    st = hipmem.Stream()
    pn = native_pp(pp)
    V = C.c_void_p
    if posed:
        pv = np.zeros(1, N.POSE_VIEW_DTYPE)
        pv["Rcw"][0], pv["tcw"][0], pv["Ow"][0] = list(Fg.Rcw), list(Fg.tcw), list(Fg.Ow)
        d_pose = hipmem.DevBuf.from_numpy(pv)
        Fg.Rcw[:] = [7.0] * 9; Fg.tcw[:] = [7.0] * 3; Fg.Ow[:] = [7.0] * 3        # not read: the pose comes from the device
        N.check(ex._h, ex._lib.hs_search_by_projection_posed_device(ex._h, C.byref(Fg), V(d_pose.ptr), V(bufs[4].ptr), L, C.byref(pn), V(d_i.ptr), V(d_d.ptr),
                                                                    V(d_n.ptr), V(st.ptr)))
    else:
        N.check(ex._h, ex._lib.hs_search_by_projection_device(ex._h, C.byref(Fg), V(bufs[4].ptr), L, C.byref(pn), V(d_i.ptr), V(d_d.ptr), V(d_n.ptr), V(st.ptr)))
    st.synchronize()
    return d_i.to_numpy(np.int32, L), d_d.to_numpy(f32, L), int(d_n.to_numpy(np.int32, 1)[0])


@pytest.mark.parametrize("posed", [False, True], ids=["device", "posed_device"])
def test_search_by_projection_device_forms(lib, matcher, posed):
    """the temporaries (d_cell, d_winner, d_pangle) come from the handle's scratch: filled on the caller's stream in front of the launches.  The device
    forms do not wait, so they are not checked for (c); a dropped rotation entry keeps match_dist, as the device form documents."""
    cases = []
    for c in area_cases():
        if len(c["fa"]["kps"]) == 0 or len(c["lms"]) == 0:
            continue
        for name in ("local map", "last frame"):
            pp = next(x[2] for x in AE.presets(matcher, float(c["th"])) if x[0] == name)
            oi, od, on = oracle.search_by_projection(c["Fo"], c["lms"], pp)

            def check(out, oi=oi, od=od, on=on):
                gi, gd, gn = out
                assert same_bits(gi, oi) and gn == on and same_bits(gd[gi >= 0], od[oi >= 0])
            cases.append((c["tag"] + (name,), functools.partial(c_projection_device, matcher, c["fa"], c["lms"], pp, posed), check))
    under_poison(lib, cases)


def test_search_by_projection_frame(lib):
    """a published extraction (keypoints and descriptors from the frame cache), landmarks of the edge-case generator; L = 300, then 1"""
    Limg, Rimg = synth_stereo_pair(23, 640, 480)
    ex = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=1000))
    m = HS.FeatureMatcher(HS.FeatureMatcherSettings(nnratio=0.8), ex)
    (kl, _), (dl, _) = ex.extract_batch([Limg, Rimg], publish=True)
    rng = np.random.default_rng(11)
    n = len(kl)
    fa = dict(Rcw=np.eye(3, dtype=f32), tcw=np.zeros(3, f32), fx=512.0, fy=512.0, cx=320.0, cy=240.0, mbf=51.2, sensor=1, bounds=(0.0, 640.0, 0.0, 480.0),
              kps=kl, desc=dl, uR=(kl["x"] - rng.uniform(1, 40, n)).astype(f32), kp_lm_obs=rng.integers(-1, 3, n).astype(np.int32), size_ref=31.0)
    lms = scenes._area_landmarks(rng, fa, rng.integers(0, n, 300), rng.choice([0, 3, 20, 50, 90], 300))
    Fo, ko = oracle.make_frame_view(oracle.FrameView, **fa)
    Fg, kg = oracle.make_frame_view(N.FrameView, **fa)
    tok = C.c_uint64(0)
    assert lib.hs_frame_find(ex.device, Fg.kps, Fg.n, C.byref(tok)) == N.HS_OK and tok.value
    cases = []
    for L in (300, 1):
        for name, _, pp in AE.presets(m, 5.0):
            want = oracle.search_by_projection(Fo, lms[:L], pp)
            cases.append(((name, L), functools.partial(c_projection, m, Fg, lms[:L], pp, tok.value), exact(*want)))
    under_poison(lib, cases)
    for t in ex.last_frame_tokens:
        ex.release_frame(t)


def c_frame_grid(m, Fg):
    ex = m._ex
    got = sentinel((Fg.n, 2), np.int8)
    N.check(ex._h, ex._lib.hs_frame_grid(ex._h, C.byref(Fg), p(got)))
    return (got.astype(np.int64),)


def test_frame_grid(lib, matcher):
    under_poison(lib, [(c["tag"], functools.partial(c_frame_grid, matcher, c["Fg"]), exact(oracle.frame_grid(c["Fo"]))) for c in area_cases()])


def c_sim3_projection(m, Fg, c):
    ex = m._ex
    lms = np.ascontiguousarray(c["lms"], N.LM_DTYPE)
    S = np.ascontiguousarray(c["Scw"], f32).reshape(16)
    taken = np.ascontiguousarray(c["kp_matched"], np.uint8).copy()
    midx, n = sentinel(len(lms), np.int32), C.c_int32(SENT)
    N.check(ex._h, ex._lib.hs_search_by_projection_sim3(ex._h, C.byref(Fg), p(S), p(lms), len(lms), int(c["th"]), float(c["th_low"]), p(taken), p(midx), C.byref(n)))
    return midx, taken, n.value


def test_search_by_projection_sim3(lib, matcher):
    """kp_matched goes in and comes back (inout); d_geo is a temporary between the two kernels"""
    cases = []
    for c in area_cases():
        want = oracle.search_by_projection_sim3(c["Fo"], c["Scw"], c["lms"], c["th"], c["th_low"], c["kp_matched"])
        cases.append((c["tag"], functools.partial(c_sim3_projection, matcher, c["Fg"], c), exact(*want)))
    under_poison(lib, cases)


def c_sim3(m, Fg1, Fg2, s):
    ex = m._ex
    l1, l2 = np.ascontiguousarray(s["lms1"], N.LM_DTYPE), np.ascontiguousarray(s["lms2"], N.LM_DTYPE)
    R, t = np.ascontiguousarray(s["R12"], f32).reshape(9), np.ascontiguousarray(s["t12"], f32).reshape(3)
    out, n = sentinel(Fg1.n, np.int32), C.c_int32(SENT)
    N.check(ex._h, ex._lib.hs_search_by_sim3(ex._h, C.byref(Fg1), p(l1), C.byref(Fg2), p(l2), float(s["s12"]), p(R), p(t), float(s["th"]), float(s["th_high"]),
                                             p(out), C.byref(n)))
    return out, n.value


def test_search_by_sim3(lib, matcher):
    cases, keep = [], []
    for c in area_cases():
        s = c["sim3"]
        F2o, k2o = oracle.make_frame_view(oracle.FrameView, **s["fb"])
        F2g, k2g = oracle.make_frame_view(N.FrameView, **s["fb"])
        keep += [F2o, k2o, F2g, k2g]
        want = oracle.search_by_sim3(c["Fo"], s["lms1"], F2o, s["lms2"], s["s12"], s["R12"], s["t12"], s["th"], s["th_high"])
        cases.append((c["tag"] + (len(s["fb"]["kps"]),), functools.partial(c_sim3, matcher, c["Fg"], F2g, s), exact(*want)))
    under_poison(lib, cases)


def test_search_for_initialization(lib, matcher):
    """d_odist and d_self are temporaries, the owner vector is an `out` piece the host merges into matches12"""
    rng = np.random.default_rng(5)
    cases, keep = [], []
    for c in area_cases():
        fa = c["fa"]
        if len(fa["kps"]) == 0:
            continue
        k1, d1, prev = AE.init_inputs(rng, fa)
        fi = dict(fa, uR=None, kp_lm_obs=None, sensor=0)
        Fo, ko = oracle.make_frame_view(oracle.FrameView, **fi)
        Fg, kg = oracle.make_frame_view(N.FrameView, **fi)
        keep += [Fo, ko, Fg, kg]
        want = oracle.search_for_initialization(k1, d1, Fo, prev, c["window"], matcher.TH_LOW, matcher.mfNNratio)
        cases.append((c["tag"] + (c["window"],), functools.partial(matcher.SearchForInitialization, k1, d1, Fg, prev, c["window"]), exact(*want)))
    under_poison(lib, cases)


# ---------------------------------------------------------------- vocabulary-grouped matchers, transform, BoW vector, 2-NN
@functools.lru_cache(None)
def bow_cases():
    rng = np.random.default_rng(77)
    scale = np.array([[1e-5, 1e-5, 1e-2], [1e-5, 1e-5, 1e-2], [1e-2, 1e-2, 1.0]])
    F = lambda: (rng.normal(0, 1, (3, 3)) * scale).astype(f32)
    return [scenes._bow_mixed(rng, 300, 300, 60, F12=None, check_rotation=1),
            scenes._bow_mixed(rng, 1, 1, 1, keep1=None, keep2=None, F12=None),
            scenes._bow_mixed(rng, 65, 65, 7, F12=F(), sigma_ref=400.0, check_rotation=1),
            scenes._bow_mixed(rng, 300, 65, 300, F12=F(), sigma_ref=1e5, check_rotation=0),
            scenes._bow_mixed(rng, 0, 5, 2, F12=None),
            scenes._bow_mixed(rng, 5, 0, 2, F12=None),
            scenes._bow_disjoint(rng, 1),                                         # nodes on one side only, empty nodes
            scenes._bow_list_sizes(rng)]


def bow_tag(c):
    return (c["kind"], len(c["k1"]), len(c["k2"]), c["F12"] is not None, c["check_rotation"])


def test_search_by_bow_ex(lib, matcher):
    """with and without F12 (the epipolar gate), with and without the rotation check (d_ang, d_self)"""
    cases = []
    for c in bow_cases():
        fvs = (c["k1"], c["d1"], c["fv1"], c["k2"], c["d2"], c["fv2"])
        want = oracle.search_by_bow(*fvs, c["keep1"], c["score_threshold"], c["ratio"], c["check_rotation"], keep2=c["keep2"], F12=c["F12"],
                                    size_ref=c["size_ref"], sigma_ref=c["sigma_ref"])
        cases.append((bow_tag(c), functools.partial(BE.native_bow, matcher, c, "ex"), exact(*want)))
    assert any(c["F12"] is not None for c in bow_cases()) and any(c["F12"] is None for c in bow_cases())
    under_poison(lib, cases)


def test_search_by_bow_legacy(lib, matcher):
    """d_taken2: the side-2 features an earlier side-1 feature matched; zeroed by the launcher"""
    cases = []
    total = 0
    for c in bow_cases():
        fvs = (c["k1"], c["d1"], c["fv1"], c["k2"], c["d2"], c["fv2"])
        want = oracle.search_by_bow_legacy(*fvs, c["keep1"], c["keep2"], c["score_threshold"], c["ratio"], c["check_rotation"])
        total += want[1]
        cases.append((bow_tag(c), functools.partial(BE.native_bow, matcher, c, "legacy"), exact(*want)))
    assert total > 50                                                            # not vacuous: a non-zero d_taken2 would lose these
    under_poison(lib, cases)


def test_bow_transform(lib, matcher):
    cases = []
    trees = [e for e in scenes.vocab_edge_trees(0) if e["name"] in ("shallow_leaf", "renumbered")]
    assert len(trees) == 2
    for e in trees:
        t = e["tree"]
        To = scenes.tree_struct(oracle.VocabTree, t)
        desc = np.ascontiguousarray(np.resize(e["desc"], (300, 32)))
        for levelsup in (1, t["levels"]):
            ow, owt, ond = oracle.bow_transform(To, desc, levelsup)               # per descriptor: a prefix is the shorter call's reference
            for n in (300, 1, 65):
                cases.append(((e["name"], levelsup, n), functools.partial(BE.host_transform, matcher, t, desc[:n], levelsup), exact(ow[:n], owt[:n], ond[:n])))
    under_poison(lib, cases)


def test_bow_vector(lib, matcher):
    """its output pieces are temporaries that come back by a count: hs_bow_vector checks the arena by itself (HsStage::verify)"""
    voc = HS.ORBVocabulary.__new__(HS.ORBVocabulary)
    voc._vocab, voc._ex = None, matcher._ex
    rng = np.random.default_rng(7)
    cases = []
    for n, n_words in ((300, 40), (1, 10), (65, 1000), (0, 10), (300, 100000)):
        word = rng.integers(0, n_words, n).astype(np.int32)
        weight = (rng.random(n) * 10 ** rng.uniform(-3, 3, n)).astype(f32)
        weight[rng.random(n) < 0.1] = 0.0
        rw, rv = RP.bow_vector(word, weight)
        cases.append(((n, n_words), functools.partial(voc.bow_vector, word, weight), exact(np.array(rw, np.int32), np.array(rv, np.float64))))
    under_poison(lib, cases)


def c_knn2(m, q, t):
    ex = m._ex
    outs = [sentinel(len(q), np.int32) for _ in range(3)]
    N.check(ex._h, ex._lib.hs_hamming_knn2(ex._h, p(q), len(q), p(t), len(t), p(outs[0]), p(outs[1]), p(outs[2])))
    return tuple(outs)


def test_hamming_knn2(lib, matcher):
    rng = np.random.default_rng(6)
    R = lambda n: rng.integers(0, 256, (n, 32), dtype=np.uint8)
    cases = []
    for nq, nt in ((300, 300), (1, 1), (65, 0), (65, 65), (1, 300), (300, 1)):
        q, t = R(nq), R(nt)
        if nq > 1 and nt > 1:
            t[:nt // 2] = scenes.flip_bits(rng, q[rng.integers(0, nq, nt // 2)], rng.integers(0, 20, nt // 2))
        cases.append(((nq, nt), functools.partial(c_knn2, matcher, q, t), exact(*oracle.hamming_knn2(q, t))))
    under_poison(lib, cases)


# ---------------------------------------------------------------- landmarks
def c_best_descriptors(m, off, desc):
    ex = m._ex
    L = len(off) - 1
    best, med = sentinel(L, np.int32), sentinel(L, np.int32)
    N.check(ex._h, ex._lib.hs_landmark_best_descriptors(ex._h, p(off), p(desc), L, p(best), p(med)))
    return best, med


def test_landmark_best_descriptors(lib, matcher):
    """N of 0, 1, 65 (the workgroup path) and 300 in one batch with an empty first, middle and last landmark; then one landmark alone"""
    rng = np.random.default_rng(3)
    E = np.zeros((0, 32), np.uint8)
    batches = [[E, LD.clustered(rng, 1), LD.clustered(rng, 65), E, LD.clustered(rng, 300, centres=4, max_flips=6), LD.clustered(rng, 40), E] +
               LD.ragged_batch(5, 300, big=[(7, 70)]), [LD.clustered(rng, 9)], LD.ragged_batch(6, 65), [E]]
    cases = []
    for lms in batches:
        off, desc = LD.csr(lms)
        cases.append(((len(lms), int(off[-1])), functools.partial(c_best_descriptors, matcher, off, desc), exact(*distinctive_descriptors_fast(lms))))
    under_poison(lib, cases)


def c_update_entries(m, ent, off, ob, doff, dflat):
    ex = m._ex
    L = len(ent)
    outs = [sentinel((L, 3), f32)] + [sentinel(L, f32) for _ in range(4)] + [sentinel(L, np.int32) for _ in range(3)]
    prm = N.LmEntryParams()
    N.check(ex._h, ex._lib.hs_landmark_update_entries(ex._h, C.byref(prm), L, p(ent), p(off), p(ob), p(doff), p(dflat), *[p(o) for o in outs]))
    return tuple(outs)


def test_landmark_update_entries(lib, matcher):
    """N_i = 0: normal, min / max and mean distance are left unchanged — they hold the 0x3C sentinel afterwards, not what the arena held"""
    left = sentinel(1, f32)[0]
    cases = []
    empties = 0
    for seed, L in ((3, 300), (4, 1), (5, 65)):
        ent, off, ob, descs = random_batch(seed, L, n_max=6, big=[(0, 70)] if L > 1 else ())
        doff, dflat = LE.desc_csr(descs)
        want = RLE.update_entries_fast(ent, off, ob, descs)
        empty = np.diff(off) == 0
        empties += int(empty.sum())

        def check(out, want=want, empty=empty):
            for o, k in zip(out, LE.KEYS):
                w = np.array(want[k], copy=True)
                if k in ("normal", "min_dist", "max_dist", "mean_dist"):
                    w[empty] = left
                assert RLE.same(o, w), k
        cases.append(((seed, L), functools.partial(c_update_entries, matcher, ent, off, ob, doff, dflat), check))
    assert empties > 0
    under_poison(lib, cases)


# ---------------------------------------------------------------- key-frame graph, local map
def votes_case(matcher, T, queries, ids, count_bad_kf, th, cap, weights):
    off, q_lm = csr(queries)
    want = RK.votes_fast(T, off, q_lm, ids, count_bad_kf, th, cap)

    def run():
        st, out = KG.c_votes(matcher, T, off, q_lm, ids, count_bad_kf, th, cap, weights=weights, fill=77)
        assert st == N.HS_OK, matcher._ex._lib.hs_orb_last_error(matcher._ex._h)
        return tuple(out[k] for k in RK.VOTE_KEYS if out[k] is not None)

    def check(out):
        got = dict(zip([k for k in RK.VOTE_KEYS if weights or k != "weights"], out))
        got.setdefault("weights", None)
        bad = RK.same(got, want, RK.VOTE_KEYS)
        assert bad is None, bad
    return run, check


def test_kf_votes(lib, matcher):
    """queries with an empty first, middle and last row; n_kf at and one above HS_KF_LDS_SLOTS with weights = NULL (the counters are a temporary of
    the arena); an ordered list of HS_KF_SORT_PASS + 1 entries with cap below and above it"""
    cases = []
    T = random_table(7, 64, 300, max_obs=40, big=[(11, 64)])
    rng = np.random.default_rng(3)
    queries = [[], rng.choice(300, 200, replace=False), [], np.arange(300), [5], []]
    for weights, cap in ((True, 10), (False, 64), (True, 3)):
        cases.append((("small", weights, cap),) + votes_case(matcher, T, queries, None, 1, 2, cap, weights))
    cases.append((("one landmark", 1),) + votes_case(matcher, table(1, [[0]]), [[0]], None, 0, 1, 4, True))
    lim = N.HS_KF_LDS_SLOTS
    for n_kf in (lim, lim + 1):
        T = random_table(n_kf, n_kf, 60, max_obs=30, big=[(0, 500)])
        T["lm_obs_kf"][int(T["lm_obs_offsets"][1]) - 1] = n_kf - 1
        ids = np.array([-1, -1, int(T["kf_id"][T["lm_obs_kf"][0]]), -1, -1], np.int64)
        cases.append((("lds limit", n_kf),) + votes_case(matcher, T, [[], np.arange(60), [0, 1, 2], np.arange(60).repeat(2), []], ids, 0, 1, 16, False))
    n = N.HS_KF_SORT_PASS + 1
    obs = [list(range(n))] + [list(range(k, n, 3)) for k in range(7)]
    T = table(2000, obs)
    for cap in (n - 1, n + 3):
        cases.append((("sort pass + 1", cap),) + votes_case(matcher, T, [list(range(len(obs)))], None, 0, 1, cap, True))
    under_poison(lib, cases)


def c_redundancy(m, T, cand, is_mono, th_obs, frac):
    ex = m._ex
    KT, keep = KG.native_table(N, T)
    Cn = len(cand["cand_slot"])
    out = [sentinel(Cn, np.int32), sentinel(Cn, np.int32), sentinel(Cn, np.uint8)]
    N.check(ex._h, ex._lib.hs_kf_redundancy(ex._h, C.byref(KT), Cn, p(cand["cand_slot"]), p(cand["cand_th_depth"]), p(cand["cand_offsets"]), p(cand["item_lm"]),
                                            p(cand["item_octave"]), p(cand["item_depth"]), is_mono, th_obs, frac, *[p(o) for o in out]))
    return tuple(out)


def test_kf_redundancy(lib, matcher):
    """candidates with no item first, in the middle and last"""
    cases = []
    for seed, L, sizes in ((9, 300, [0, 65, 0, 300, 1, 0]), (10, 1, [1]), (11, 65, [0]), (12, 300, [300, 64])):
        T = random_table(seed, 80, L, max_obs=40, big=[(0, 70)])
        cand = random_candidates(seed, T, sizes)
        for is_mono, th_obs, frac in ((0, 3, 0.9), (1, 1, 0.05)):
            w = RK.redundancy_fast(T, cand["cand_slot"], cand["cand_th_depth"], cand["cand_offsets"], cand["item_lm"], cand["item_octave"], cand["item_depth"],
                                   is_mono, th_obs, frac)
            cases.append(((seed, L, is_mono), functools.partial(c_redundancy, matcher, T, cand, is_mono, th_obs, frac), exact(*[w[k] for k in RK.RED_KEYS])))
    under_poison(lib, cases)


def c_local_keyframes(m, c):
    ex = m._ex
    w, bad, par = (np.ascontiguousarray(c[k], d) for k, d in (("weights", np.int32), ("kf_bad", np.uint8), ("parent", np.int32)))
    n_kf = len(w)
    ng = np.ascontiguousarray(c["neigh"], np.int32).reshape(n_kf, -1) if n_kf else np.zeros((0, 0), np.int32)
    local, n_local = sentinel(n_kf, np.uint8), sentinel(1, np.int32)
    N.check(ex._h, ex._lib.hs_local_keyframes(ex._h, n_kf, p(w), p(bad), p(ng), ng.shape[1], p(par), int(c["n_max"]), int(c["n_neighbor"]), p(local), p(n_local)))
    return local, int(n_local[0])


def test_local_keyframes(lib, matcher):
    cases = []
    for seed, n_kf in ((1, 300), (2, 1), (3, 65), (4, 300), (5, 64)):
        c = random_keyframes(1000 * n_kf + seed, n_kf, neigh_cap=(1, 10, 70)[seed % 3])
        want = RL.local_keyframes_fast(c["weights"], c["kf_bad"], c["neigh"], c["parent"], c["n_max"], c["n_neighbor"])
        cases.append(((seed, n_kf), functools.partial(c_local_keyframes, matcher, c), exact(*want)))
    empty = dict(weights=np.zeros(0, np.int32), kf_bad=np.zeros(0, np.uint8), neigh=np.zeros((0, 0), np.int32), parent=np.zeros(0, np.int32), n_max=80, n_neighbor=0)
    cases.append((("no key frame",), functools.partial(c_local_keyframes, matcher, empty), exact(np.zeros(0, np.uint8), 0)))
    under_poison(lib, cases)


def c_local_points(m, T, local, flm, cap):
    ex = m._ex
    KT, keep = KG.native_table(N, T)
    loc, flm = np.ascontiguousarray(local, np.uint8), np.ascontiguousarray(flm, np.int32)
    rem, sel, n_sel = sentinel(len(flm), np.uint8), sentinel(cap, np.int32), sentinel(1, np.int32)
    N.check(ex._h, ex._lib.hs_local_points(ex._h, C.byref(KT), p(loc), p(flm), len(flm), p(rem), p(sel), cap, p(n_sel)))
    return rem, sel, int(n_sel[0])


def test_local_points(lib, matcher):
    """the keep flags and the block counts are a temporary (d_work); cap below, at and above n_sel; L in one and in two compaction blocks; an observation
    table with an empty first, middle and last row"""
    cases = []
    B = N.HS_LOCAL_POINTS_BLOCK
    tables = [random_points(L + 5, 65, L, max_obs=12, big=[(0, 65)] if L else (), n_assoc=300 if L else 7, p_local=0.15) for L in (300, 1, 65, 0, B + 1)]
    tables[1][0]["lm_bad"][0], tables[1][2][:] = 0, -1                              # the one landmark is selected
    T = table(4, [[], [0, 1], [], [2], [3], []])
    tables.append((T, np.array([1, 0, 1, 0], np.uint8), np.array([-1, 1, 4, -1], np.int32)))
    selected = 0
    for T, local, flm in tables:
        L = len(T["lm_bad"])
        n = RL.local_points_fast(T, local, flm, L)["n_sel"]
        selected += n
        for cap in sorted({max(n - 1, 0), n, n + 3}):
            want = RL.local_points_fast(T, local, flm, cap)
            cases.append(((L, cap, n), functools.partial(c_local_points, matcher, T, local, flm, cap), exact(*[want[k] for k in RL.POINT_KEYS])))
    assert selected > 100
    under_poison(lib, cases)


# ---------------------------------------------------------------- pose-only optimisation
def test_pose_optimize(lib, matcher):
    """(a) holds to the tolerance of tests/test_gpu_poseopt.py, (b) exactly.  The middle problem has two edges and does not run: its `inout` flags
    come back as they went (run_host's 0x55)."""
    golden = P.load_golden()
    ex, tau = matcher._ex, float(golden["tau"])
    names = (P.BATCH[0], None, P.BATCH[2])
    T0, cam0, e0 = P.too_few(2)
    batch = [PO.item(golden, names[0]), (T0, cam0, e0), PO.item(golden, names[2])]
    off = np.cumsum([0] + [len(e) for _, _, e in batch])

    def check_named(r, flags, name):
        g = lambda k: golden[name + "." + k]
        assert np.array_equal(flags, g("outlier"))
        assert [int(r[k]) for k in ("n_good", "n_edges", "rounds", "status")] == [int(g(k)) for k in ("n_good", "n_edges", "rounds", "status")]
        assert float(np.abs(r["Tcw_d"].reshape(4, 4) - g("Tcw_d")).max()) <= tau
        assert r["Tcw"].tobytes() == r["Tcw_d"].astype(f32).tobytes()

    def check_batch(out):
        res, outlier = out
        for q, name in enumerate(names):
            r, flags = res[q], outlier[off[q]:off[q + 1]]
            if name is not None:
                check_named(r, flags, name)
                continue
            assert (flags == 0x55).all() and len(flags) == 2
            assert [int(r[k]) for k in ("n_edges", "n_good", "rounds", "lm_iterations", "lm_trials", "status")] == [2, 0, 0, 0, 0, N.HS_POSE_TOO_FEW]
            assert r["Tcw"].tobytes() == T0.tobytes() and r["Tcw_d"].tobytes() == T0.astype(np.float64).tobytes()

    cases = [("batch 257 / 2 / 12", functools.partial(PO.run_host, ex, batch), check_batch)]
    for name in ("n1000", "n3"):
        cases.append((name, functools.partial(PO.run_host, ex, [PO.item(golden, name)]), lambda out, name=name: check_named(out[0][0], out[1], name)))
    under_poison(lib, cases)


# ---------------------------------------------------------------- allocation poison: handles and databases created after the switch is set
NF = 1000
W0, H0 = 320, 240


def per_byte_fresh(lib, build):
    """build() -> (tag, run, check) list on handles it creates itself; called once per byte, after the switch is set"""
    before = lib.hs_debug_poison_violations()
    seen = []
    try:
        for byte in BYTES:
            assert lib.hs_debug_poison(byte) == N.HS_OK
            outs = []
            for tag, run, check in build():
                out = run()
                try:
                    check(out)
                except AssertionError as e:
                    raise AssertionError("%s under allocation poison 0x%02X: %s" % (tag, byte, e)) from None
                outs.append((tag, tuple(raw(o) for o in out)))
            seen.append(outs)
    finally:
        lib.hs_debug_poison(-1)
    assert len(seen[0]) > 0 and seen[0] == seen[1], "the outputs under 0x00 and 0xFF differ"
    assert seen[0] == seen[2], "the outputs under 0x00 and 0xA5 differ"
    assert lib.hs_debug_poison_violations() == before


@functools.lru_cache(None)
def extractor_refs():
    prm = oracle.default_params(NF)
    small = synth_image(11, W0, H0)
    pair = synth_stereo_pair(80, W0, H0)
    colour = np.ascontiguousarray(np.stack([synth_image(60 + 7 * c, 2 * W0, 2 * H0) for c in range(3)], axis=2))
    grey = oracle.preprocess(colour, True, 0.5)
    return dict(small=small, small_ref=oracle.extract(prm, small), pair=pair,
                pair_ref=oracle.stereo_frontend(prm, oracle.stereo_params(fx=250.0, mbf=30.0, n_rows=H0), *pair),
                colour=colour, grey=grey, colour_ref=oracle.extract(prm, grey))


def test_extractor_under_allocation_poison(lib):
    """a fresh handle per byte: extract_batch of one 320 x 240 frame, one stereo ticket through submit_batch / wait, extract_camera_batch with the grey
    frame coming back — against oracle.extract / oracle.stereo_frontend / oracle.preprocess, as tests/test_gpu_workspace_regrow.py"""
    r = extractor_refs()
    assert len(r["small_ref"][0]) > 200 and (r["pair_ref"][5] > 0).sum() > 20

    def build():
        ex = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=NF))
        sp = HS.stereo_params(HS.Camera(fx=250.0, mbf=30.0, mnMaxY=float(H0)))

        def extract():
            k, d = ex.extract_batch([r["small"]])
            return k[0], d[0]

        def ticket():
            n, k, d, u, z = ex.wait(ex.submit_batch(list(r["pair"]), sp))
            return k[0, :n[0]], d[0, :n[0]], k[1, :n[1]], d[1, :n[1]], u[0, :n[0]], z[0, :n[0]]

        def camera():
            k, d, grey = ex.extract_camera_batch([r["colour"]], True, 0.5, want_grey=True)
            return k[0], d[0], grey[0]

        def feats(out, ref):
            for i in range(0, len(ref) - len(ref) % 2, 2):
                assert len(out[i]) == len(ref[i]) and raw(out[i]) == raw(ref[i]) and np.array_equal(out[i + 1], ref[i + 1]), i
        return [("extract_batch", extract, lambda out: feats(out, r["small_ref"])),
                ("stereo ticket", ticket, lambda out: (feats(out[:4], r["pair_ref"][:4]), exact(*r["pair_ref"][4:])(out[4:]))),
                ("extract_camera_batch", camera, lambda out: (feats(out[:2], r["colour_ref"]), exact(r["grey"])(out[2:]))),
                ("extract_batch again", extract, lambda out: feats(out, r["small_ref"]))]
    per_byte_fresh(lib, build)


def test_place_recognizer_under_allocation_poison(lib):
    """a fresh database per byte: add, erase, add again (new slots), a relocalisation and a loop query, against tests/ref_place.py"""
    sc = random_scene(21, 120, 1000, (5, 60), n_queries=4)
    assert {q["mode"] for q in sc["queries"]} == {"reloc", "loop"}
    back = {e[0]: e for e in sc["entries"]}
    gone = [e[0] for e in sc["entries"] if e[0] not in sc["erased"]][10:40:3]
    ref = scene_ref(RP, sc)
    for k in gone:
        ref.erase(k)
    for k in gone[:5]:
        ref.add(*back[k])
    wants = [ref_query(ref, sc, q) for q in sc["queries"]]

    def build():
        ex = HS.ORBExtractor(device=0)
        rec = PL.fill(HS, ex, 1000, sc["entries"], sc["erased"])
        for k in gone:
            rec.erase(k)
        for k in gone[:5]:
            assert rec.add(k, back[k][1:]) >= 120
        cases = []
        for i, (q, (want_keys, det)) in enumerate(zip(sc["queries"], wants)):
            def run(q=q):
                keys, got = PL.gpu_query(rec, q, sc["neigh"])
                return (np.array(keys, np.int64),) + tuple(got[k] for k in ("words", "score", "acc", "best"))

            def check(out, want_keys=want_keys, det=det, i=i):
                PL.assert_query(rec, out[0].tolist(), dict(zip(("words", "score", "acc", "best"), out[1:])), want_keys, det, i)
            cases.append(((i, q["mode"]), run, check))
        return cases
    per_byte_fresh(lib, build)


def test_device_vocabulary_under_allocation_poison(lib):
    """hs_vocab_upload + hs_bow_transform_device + hs_records_bow_match_device (its grow-only scratch) at the shapes of tests/test_gpu_bow_edges.py:
    the first edge tree, record sets of 5 x 301 and then 2 x 64 (the scratch is reused)"""
    e = next(iter(scenes.vocab_edge_trees(0)))
    t, desc, levelsup = e["tree"], e["desc"], 1
    To = scenes.tree_struct(oracle.VocabTree, t)
    ow, owt, ond = oracle.bow_transform(To, desc, levelsup)
    sets = list(scenes.record_edge_sets(40, pool=t["desc"]))
    picked = [sets[5], sets[3]]
    want_rec = [BE.records_bow_oracle(t, levelsup, rs, 50.0, 0.9, 1) for rs in picked]
    assert sum(int(w[1].sum()) for w in want_rec) > 50

    def build():
        ex = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=500))
        m = HS.FeatureMatcher(HS.FeatureMatcherSettings(nnratio=0.8), ex)
        voc = DeviceVocabulary(ex, scenes.tree_struct(N.VocabTree, t), levelsup, keepalive=t)
        stream = hipmem.Stream()
        d_desc = hipmem.DevBuf.from_numpy(desc)
        cases = [("transform_device", lambda: BE.device_transform(m, voc, d_desc, len(desc), None, stream), exact(ow, owt.view(np.uint32), ond))]
        for rs, want in zip(picked, want_rec):
            d_rec = hipmem.DevBuf.from_numpy(rs["buf"])
            cases.append((("records", rs["world"], rs["cap"]), functools.partial(BE.records_bow_gpu, voc, rs, d_rec, 50.0, 0.9, 1, stream), exact(*want)))
        return cases
    per_byte_fresh(lib, build)


# ---------------------------------------------------------------- the detector itself
def test_selftest_reports_its_overrun_and_the_switch_goes_off(lib, matcher):
    """the check cannot pass vacuously: a store just past the end of a staged piece (into its own padding) is reported, once; with the switch off
    afterwards a plain call returns HS_OK and the counter stays"""
    ex = matcher._ex
    rep = C.c_int(-1)
    assert lib.hs_debug_poison(-1) == N.HS_OK
    assert lib.hs_debug_poison_selftest(ex._h, C.byref(rep)) == N.HS_ERR_INVALID and rep.value == 0          # off: refused
    assert lib.hs_debug_poison(256) == N.HS_ERR_INVALID and lib.hs_debug_poison(-2) == N.HS_ERR_INVALID
    try:
        for byte in BYTES:
            before = lib.hs_debug_poison_violations()
            assert lib.hs_debug_poison(byte) == N.HS_OK
            rep = C.c_int(-1)
            assert lib.hs_debug_poison_selftest(ex._h, C.byref(rep)) == N.HS_OK and rep.value == 1, hex(byte)
            msg = ex._lib.hs_orb_last_error(ex._h).decode()
            assert "piece 0" in msg and "offset 64" in msg, msg
            assert lib.hs_debug_poison_violations() == before + 1
    finally:
        lib.hs_debug_poison(-1)
    before = lib.hs_debug_poison_violations()
    q = np.arange(64, dtype=np.uint8).reshape(2, 32)
    got = c_knn2(matcher, q, q)
    assert exact(*oracle.hamming_knn2(q, q))(got) is None
    assert lib.hs_debug_poison_violations() == before
