"""GPU parity of the vocabulary-grouped matchers, the vocabulary transform and the brute-force 2-NN on the edge cases of tests/scenes.py
(bow_edge_cases, bow_size_cases, vocab_edge_trees, knn2_edge_cases, record_edge_sets): hs_search_by_bow, hs_search_by_bow_ex,
hs_search_by_bow_legacy, hs_bow_transform, hs_vocab_upload / hs_vocab_dev_groups / hs_bow_transform_device, hs_records_bow_match_device,
hs_hamming_knn2, hs_hamming_knn2_device, hs_records_knn2_device.  Bit-exact against the oracle and, wherever it runs, against the numpy
restatement (tests/ref_bow.py).  One handle and one hs_vocab_dev per (tree, levelsup) serve all cases, in an order that shrinks and grows their
scratch.  What the entry points refuse on the host is tested as a refusal; nothing outside their contracts reaches the device.
The C++ adaptor (hyslam_amd/host/HipFeatureMatcher.h) is not driven from here: tests/cpp/test_matcher_adaptor.cpp builds its scenes in code."""
import ctypes as C

import numpy as np
import pytest

import hipmem
import oracle
import ref_bow
import scenes
import hyslam_amd as HS
from hyslam_amd import _native as N
from hyslam_amd.distributed import DeviceVocabulary, pack_record, record_bytes

pytestmark = pytest.mark.gpu
f32 = np.float32
PATTERN = 0x5A5A5A5A


@pytest.fixture(scope="module")
def matcher(gpu):
    return HS.FeatureMatcher(HS.FeatureMatcherSettings(nnratio=0.8), HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=500)))


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def fv_arrays(fv):
    return [np.ascontiguousarray(x, np.int32) for x in fv]


def native_bow(m, c, which):
    """hs_search_by_bow / _ex / _legacy through _native: every parameter of the C ABI"""
    ex = m._ex
    k1, k2 = np.ascontiguousarray(c["k1"], N.KP_DTYPE), np.ascontiguousarray(c["k2"], N.KP_DTYPE)
    d1, d2 = np.ascontiguousarray(c["d1"], np.uint8), np.ascontiguousarray(c["d2"], np.uint8)
    a, b = fv_arrays(c["fv1"]), fv_arrays(c["fv2"])
    out = np.full(len(k1), PATTERN, np.int32)
    n = C.c_int32(-7)
    head = (ex._h, p(k1), p(d1), len(k1), p(a[0]), p(a[1]), p(a[2]), len(a[0]), p(k2), p(d2), len(k2), p(b[0]), p(b[1]), p(b[2]), len(b[0]))
    Fm = None if c["F12"] is None else np.ascontiguousarray(c["F12"], f32).reshape(9)
    if which == "plain":
        st = ex._lib.hs_search_by_bow(*head, p(c["keep1"]), c["score_threshold"], c["ratio"], c["check_rotation"], p(out), C.byref(n))
    elif which == "ex":
        st = ex._lib.hs_search_by_bow_ex(*head, p(c["keep1"]), p(c["keep2"]), p(Fm), c["size_ref"], c["sigma_ref"], c["score_threshold"], c["ratio"],
                                         c["check_rotation"], p(out), C.byref(n))
    else:
        st = ex._lib.hs_search_by_bow_legacy(*head, p(c["keep1"]), p(c["keep2"]), c["score_threshold"], c["ratio"], c["check_rotation"], p(out), C.byref(n))
    N.check(ex._h, st)
    return out, n.value


def check_bow_case(m, c, with_ref=True, mirror=True):
    tag = (c["kind"], len(c["k1"]), len(c["k2"]), c["score_threshold"], c["ratio"], c["check_rotation"])
    fvs = (c["k1"], c["d1"], c["fv1"], c["k2"], c["d2"], c["fv2"])
    # hs_search_by_bow_ex: everything the case carries
    om, on = oracle.search_by_bow(*fvs, c["keep1"], c["score_threshold"], c["ratio"], c["check_rotation"], keep2=c["keep2"], F12=c["F12"],
                                  size_ref=c["size_ref"], sigma_ref=c["sigma_ref"])
    gm, gn = native_bow(m, c, "ex")
    assert np.array_equal(gm, om) and gn == on, tag + ("ex",)
    if with_ref:
        pm, pn = ref_bow.search_by_bow(*fvs, c["keep1"], c["score_threshold"], c["ratio"], c["check_rotation"], keep2=c["keep2"], F12=c["F12"],
                                       size_ref=c["size_ref"], sigma_ref=c["sigma_ref"])
        assert np.array_equal(gm, pm) and gn == pn, tag + ("ex, numpy reference",)
    if mirror:                                                                   # the same through the Python mirror (TH_LOW and nnratio from the settings)
        mm = HS.FeatureMatcher(HS.FeatureMatcherSettings(nnratio=c["ratio"], TH_LOW=c["score_threshold"], checkOri=bool(c["check_rotation"])), m._ex)
        xm, xn = mm.SearchByBoW(*fvs, c["keep1"], bool(c["check_rotation"]), keep2=c["keep2"], F12=c["F12"], size_ref=c["size_ref"], sigma_ref=c["sigma_ref"])
        assert np.array_equal(xm, om) and xn == on, tag + ("mirror",)
        if c["F12"] is not None and c["check_rotation"]:
            xm, xn = mm.SearchForTriangulation(*fvs, c["F12"], c["keep1"], c["keep2"], c["size_ref"], c["sigma_ref"])
            wm, wn = oracle.search_by_bow(*fvs, c["keep1"], c["score_threshold"], 1.0, 1, keep2=c["keep2"], F12=c["F12"], size_ref=c["size_ref"], sigma_ref=c["sigma_ref"])
            assert np.array_equal(xm, wm) and xn == wn, tag + ("triangulation",)
        xm, xn = mm.SearchByBoWLegacy(*fvs, c["keep1"], c["keep2"])
        wm, wn = oracle.search_by_bow_legacy(*fvs, c["keep1"], c["keep2"], c["score_threshold"], c["ratio"], c["check_rotation"])
        assert np.array_equal(xm, wm) and xn == wn, tag + ("legacy mirror",)
    # hs_search_by_bow: side-1 index criterion only, no gate
    om, on = oracle.search_by_bow(*fvs, c["keep1"], c["score_threshold"], c["ratio"], c["check_rotation"])
    gm, gn = native_bow(m, c, "plain")
    assert np.array_equal(gm, om) and gn == on, tag + ("plain",)
    if with_ref:
        pm, pn = ref_bow.search_by_bow(*fvs, c["keep1"], c["score_threshold"], c["ratio"], c["check_rotation"])
        assert np.array_equal(gm, pm) and gn == pn, tag + ("plain, numpy reference",)
    # hs_search_by_bow_legacy
    om, on = oracle.search_by_bow_legacy(*fvs, c["keep1"], c["keep2"], c["score_threshold"], c["ratio"], c["check_rotation"])
    gm, gn = native_bow(m, c, "legacy")
    assert np.array_equal(gm, om) and gn == on, tag + ("legacy",)
    if with_ref:
        pm, pn = ref_bow.search_by_bow_legacy(*fvs, c["keep1"], c["keep2"], c["score_threshold"], c["ratio"], c["check_rotation"])
        assert np.array_equal(gm, pm) and gn == pn, tag + ("legacy, numpy reference",)


@pytest.mark.parametrize("block", range(3))
def test_bow_edge_cases_all_entry_points(matcher, block):
    for seed in scenes.BOW_GPU_SEEDS[4 * block:4 * block + 4]:
        for case in scenes.bow_edge_cases(seed):
            check_bow_case(matcher, case)


def test_bow_size_extremes_all_entry_points(matcher):
    """n1 / n2 of 0, 1, 65 535 and above, no node on one side, one node holding everything, as many nodes as features: in an order that shrinks
    and grows the handle's scratch.  Above 2000 features the oracle alone is the expectation."""
    cases = list(scenes.bow_size_cases(3))
    for i in (6, 0, 4, 2, 7, 1, 5, 3):
        c = cases[i]
        check_bow_case(matcher, c, with_ref=max(len(c["k1"]), len(c["k2"])) <= scenes.BOW_PYREF_MAX_N, mirror=i in (4, 2))


def test_no_candidate_is_no_match_under_any_threshold(matcher):
    """DESIGN.md D10 on the device: threshold +inf, ratio 2, features without a candidate (empty list, masked out, taken)"""
    bits, kps = scenes.desc_bits, scenes.plain_kps
    d1 = np.zeros((4, 32), np.uint8)
    d2 = np.stack([bits(0), bits(*range(200))])
    c = dict(kind="d10", k1=kps(4), d1=d1, k2=kps(2), d2=d2, keep1=None, keep2=np.array([0, 1], np.uint8), F12=None, size_ref=31.0, sigma_ref=1.0,
             fv1=(np.array([1, 2, 3], np.int32), np.array([0, 1, 2, 4], np.int32), np.array([0, 1, 2, 3], np.int32)),
             fv2=(np.array([1, 2, 3], np.int32), np.array([0, 0, 1, 2], np.int32), np.array([0, 1], np.int32)),
             score_threshold=float(np.inf), ratio=2.0, check_rotation=1)
    assert native_bow(matcher, c, "ex")[0].tolist() == [-1, -1, 1, 1] and native_bow(matcher, c, "legacy")[0].tolist() == [-1, -1, 1, -1]
    check_bow_case(matcher, c)


def test_bow_refusals(matcher):
    """what the host entry points refuse before anything is launched: indices outside [0, n), a node_ptr that is negative or decreases, missing arrays"""
    c = next(x for x in scenes.bow_edge_cases(1) if x["kind"] == "list_sizes")
    assert len(c["fv1"][0]) >= 3 and len(c["fv2"][0]) >= 3                        # at least three nodes per side: node_ptr has an inner entry
    ex = matcher._ex
    for side, bad in (("fv1", len(c["k1"])), ("fv1", -1), ("fv2", len(c["k2"])), ("fv2", -2)):
        idx = c[side][2].copy(); idx[len(idx) // 2] = bad
        for which in ("plain", "ex", "legacy"):
            with pytest.raises(N.HsError) as e:
                native_bow(matcher, dict(c, **{side: (c[side][0], c[side][1], idx)}), which)
            assert e.value.status == N.HS_ERR_INVALID
    empty = dict(c, k2=c["k2"][:0], d2=c["d2"][:0], keep2=None)                  # nothing would be launched: node_ptr is checked all the same
    for side in ("fv1", "fv2"):
        neg = c[side][1].copy(); neg[0] = -1
        dec = c[side][1].copy(); dec[1] = dec[-1] + 1                             # node_ptr[1] > node_ptr[2]
        assert dec[1] > dec[2]
        for ptr in (neg, dec):
            for which in ("plain", "ex", "legacy"):
                for base in (c, empty):
                    with pytest.raises(N.HsError) as e:
                        native_bow(matcher, dict(base, **{side: (c[side][0], ptr, c[side][2])}), which)
                    assert e.value.status == N.HS_ERR_INVALID
    n = C.c_int32()
    k, d = np.ascontiguousarray(c["k1"], N.KP_DTYPE), np.ascontiguousarray(c["d1"])
    a = fv_arrays(c["fv1"])
    assert ex._lib.hs_search_by_bow(ex._h, p(k), p(d), len(k), p(a[0]), p(a[1]), p(a[2]), len(a[0]), p(k), p(d), len(k), p(a[0]), p(a[1]), p(a[2]), len(a[0]),
                                    None, 50.0, 0.8, 1, None, C.byref(n)) == N.HS_ERR_INVALID       # no match12
    assert ex._lib.hs_search_by_bow(ex._h, p(k), p(d), -1, p(a[0]), p(a[1]), p(a[2]), len(a[0]), p(k), p(d), len(k), p(a[0]), p(a[1]), p(a[2]), len(a[0]),
                                    None, 50.0, 0.8, 1, p(np.zeros(len(k), np.int32)), C.byref(n)) == N.HS_ERR_INVALID
    check_bow_case(matcher, c)                                                   # the handle is as good as before


# ---------------------------------------------------------------- vocabulary transform
def host_transform(m, tree, desc, levelsup):
    ex = m._ex
    T = scenes.tree_struct(N.VocabTree, tree)
    n = len(desc)
    w = np.full(n, PATTERN, np.int32); wt = np.zeros(n, f32); nd = np.full(n, PATTERN, np.int32)
    N.check(ex._h, ex._lib.hs_bow_transform(ex._h, C.byref(T), p(desc), n, levelsup, p(w), p(wt), p(nd)))
    return w, wt, nd


def device_transform(m, voc, d_desc, n_max, count, stream):
    """hs_bow_transform_device on a caller stream; count None = d_n NULL.  -> the three output arrays of n_max entries, pre-filled with a pattern"""
    outs = [hipmem.DevBuf(n_max * 4, zero=False) for _ in range(3)]
    for o in outs:
        o.fill(0x5A)
    d_n = None if count is None else hipmem.DevBuf.from_numpy(np.array([count], np.int32))
    voc.transform_device(d_desc.ptr, d_n.ptr if d_n else 0, n_max, outs[0].ptr, outs[1].ptr, outs[2].ptr, stream.ptr)
    stream.synchronize()
    return outs[0].to_numpy(np.int32, n_max), outs[1].to_numpy(np.uint32, n_max), outs[2].to_numpy(np.int32, n_max)


@pytest.fixture(scope="module")
def edge_trees(matcher):
    """every edge tree with one DeviceVocabulary per levelsup it accepts"""
    out = []
    for e in scenes.vocab_edge_trees(0):
        T = scenes.tree_struct(N.VocabTree, e["tree"])
        vocs = {}
        for levelsup in e["levelsups"]:
            if levelsup in e["upload_refused"]:
                v = C.c_void_p()
                assert matcher._ex._lib.hs_vocab_upload(matcher._ex._h, C.byref(T), levelsup, C.byref(v)) == N.HS_ERR_INVALID and not v.value
            else:
                vocs[levelsup] = DeviceVocabulary(matcher._ex, T, levelsup, keepalive=e["tree"])
        out.append((e, vocs))
    yield out
    for e, vocs in out:
        for v in vocs.values():
            v.close()


def test_transform_on_edge_trees(matcher, edge_trees):
    """hs_bow_transform and hs_bow_transform_device (d_n NULL, in range, negative, above n_max) on every edge tree and levelsup; hs_vocab_dev_groups
    against the reference's count of feature-vector nodes; a tree with 8193 nodes at the feature-vector level is refused (in the fixture)"""
    stream = hipmem.Stream()
    for e, vocs in edge_trees:
        t, desc = e["tree"], e["desc"]
        To = scenes.tree_struct(oracle.VocabTree, t)
        d_desc = hipmem.DevBuf.from_numpy(desc)
        n = len(desc)
        for levelsup in e["levelsups"]:
            ow, owt, ond = oracle.bow_transform(To, desc, levelsup)
            pw, pwt, pnd = ref_bow.bow_transform(t, desc, levelsup)
            gw, gwt, gnd = host_transform(matcher, t, desc, levelsup)
            tag = (e["name"], levelsup)
            assert np.array_equal(gw, ow) and np.array_equal(gwt.view(np.uint32), owt.view(np.uint32)) and np.array_equal(gnd, ond), tag
            assert np.array_equal(gw, pw) and np.array_equal(gwt.view(np.uint32), pwt.view(np.uint32)) and np.array_equal(gnd, pnd), tag + ("numpy reference",)
            if levelsup not in vocs:
                continue
            assert vocs[levelsup].groups == ref_bow.feature_vector_nodes(t, levelsup), tag
            for count in (None, n // 2, -3, n + 100, 0, 1):
                seen = n if count is None else min(max(count, 0), n)
                dw, dwt, dnd = device_transform(matcher, vocs[levelsup], d_desc, n, count, stream)
                assert np.array_equal(dw[:seen], ow[:seen]) and np.array_equal(dwt[:seen], owt.view(np.uint32)[:seen]) and np.array_equal(dnd[:seen], ond[:seen]), tag + (count,)
                assert (dw[seen:] == PATTERN).all() and (dwt[seen:] == PATTERN).all() and (dnd[seen:] == PATTERN).all(), tag + (count, "beyond the count")


def test_host_and_device_transform_agree_across_the_block_boundary(matcher, edge_trees):
    """hs_bow_transform runs the device-vocabulary kernel (k_bow_transform_dev, 256 descriptors per block) with a tree that has neither groups nor
    reported ids: on every edge tree without orig_id, n = 1, 255, 256, 257 descriptors give the same word, weight and node arrays through
    hs_bow_transform and hs_bow_transform_device, and both equal the numpy reference's"""
    stream = hipmem.Stream()
    sizes = (1, 255, 256, 257)
    seen_trees = 0
    for e, vocs in edge_trees:
        t = e["tree"]
        if t["orig_id"] is not None:
            continue
        seen_trees += 1
        desc = np.ascontiguousarray(np.resize(e["desc"], (max(sizes), 32)))     # the tree's own descriptors, repeated
        for levelsup, voc in vocs.items():
            pw, pwt, pnd = ref_bow.bow_transform(t, desc, levelsup)               # per descriptor: a prefix is the shorter call's reference
            for n in sizes:
                d_desc = hipmem.DevBuf.from_numpy(desc[:n])
                gw, gwt, gnd = host_transform(matcher, t, desc[:n], levelsup)
                dw, dwt, dnd = device_transform(matcher, voc, d_desc, n, None, stream)
                tag = (e["name"], levelsup, n)
                assert np.array_equal(gw, dw) and np.array_equal(gwt.view(np.uint32), dwt) and np.array_equal(gnd, dnd), tag
                assert np.array_equal(gw, pw[:n]) and np.array_equal(gwt.view(np.uint32), pwt.view(np.uint32)[:n]) and np.array_equal(gnd, pnd[:n]), tag + ("numpy reference",)
    assert seen_trees >= 4


def test_transform_refusals(matcher):
    """trees that are not forward-linked, a root without children, missing arrays: HS_ERR_INVALID from hs_bow_transform and hs_vocab_upload"""
    e = next(iter(scenes.vocab_edge_trees(3)))
    ex = matcher._ex
    desc = e["desc"][:4]
    out = [np.zeros(4, np.int32), np.zeros(4, f32), np.zeros(4, np.int32)]

    def both(tree):
        T = scenes.tree_struct(N.VocabTree, tree)
        v = C.c_void_p()
        a = ex._lib.hs_bow_transform(ex._h, C.byref(T), p(desc), 4, 1, p(out[0]), p(out[1]), p(out[2]))
        b = ex._lib.hs_vocab_upload(ex._h, C.byref(T), 1, C.byref(v))
        assert not v.value
        return a, b
    t = e["tree"]
    parent = int(np.nonzero(t["child_count"] > 0)[0][-1])
    for key, idx, val in (("child_begin", parent, parent), ("child_begin", parent, 0), ("child_count", parent, t["n_nodes"]), ("child_count", 2, -1),
                          ("child_count", 0, 0)):
        bad = dict(t, **{key: t[key].copy()}); bad[key][idx] = val
        assert both(bad) == (N.HS_ERR_INVALID, N.HS_ERR_INVALID), (key, idx, val)
    assert both(dict(t, n_nodes=1)) == (N.HS_ERR_INVALID, N.HS_ERR_INVALID) and both(dict(t, levels=0)) == (N.HS_ERR_INVALID, N.HS_ERR_INVALID)
    gw, gwt, gnd = host_transform(matcher, t, e["desc"], 1)
    assert np.array_equal(gw, ref_bow.bow_transform(t, e["desc"], 1)[0])


# ---------------------------------------------------------------- frame records
def records_bow_gpu(voc, rs, d_rec, thr, ratio, rot, stream):
    world, cap = rs["world"], rs["cap"]
    d_m, d_n = hipmem.DevBuf(world * cap * 4, zero=False), hipmem.DevBuf(world * 4, zero=False)
    d_m.fill(0x5A); d_n.fill(0x5A)
    voc.records_bow_match_device(d_rec.ptr, rs["stride"], world, rs["rank"], cap, thr, ratio, rot, d_m.ptr, d_n.ptr, stream.ptr)
    stream.synchronize()
    return d_m.to_numpy(np.int32, world * cap).reshape(world, cap), d_n.to_numpy(np.int32, world)


def records_bow_oracle(tree, levelsup, rs, thr, ratio, rot):
    To = scenes.tree_struct(oracle.VocabTree, tree)
    world, cap, rank = rs["world"], rs["cap"], rs["rank"]
    fvs = [ref_bow.feature_vector(*oracle.bow_transform(To, d, levelsup)) for k, d in rs["frames"]]
    out = np.full((world, cap), -1, np.int32); nm = np.zeros(world, np.int32)
    k1, d1 = rs["frames"][rank]
    for q in range(world):
        if q != rank:
            m, nm[q] = oracle.search_by_bow(k1, d1, fvs[rank], rs["frames"][q][0], rs["frames"][q][1], fvs[q], None, thr, ratio, rot)
            out[q, :len(m)] = m
    return out, nm


RECORD_ORDER = (5, 0, 7, 1, 6, 2, 4, 3)           # large, small, the cap = 65 535 set, small ...: every hs_vocab_dev's scratch shrinks and grows


def test_records_bow_match_on_edge_trees(matcher, edge_trees):
    """hs_records_bow_match_device on every record set, every edge tree and every levelsup the tree was uploaded with: 1 group (levelsup >= L),
    group counts that are not multiples of 1024, 8192 groups; empty records, header counts of -5 and cap + 1000 (clamped on the device), strides
    above hs_record_bytes(cap).  Rows beyond the count and the `rank` row are -1, n_matches[rank] == 0.  The cap = 65 535 set has the oracle
    alone as its expectation, every other set the numpy reference too."""
    stream = hipmem.Stream()
    total = 0
    for ti, (e, vocs) in enumerate(edge_trees):
        t = e["tree"]
        sets = list(scenes.record_edge_sets(40 + ti, pool=t["desc"]))
        for levelsup, voc in vocs.items():
            thr, ratio, rot = [(50.0, 0.9, 1), (50.0, 1.0, 0), (30.5, 1.5, 1)][(ti + levelsup) % 3]
            for si in RECORD_ORDER:
                rs = sets[si]
                d_rec = hipmem.DevBuf.from_numpy(rs["buf"])
                gm, gn = records_bow_gpu(voc, rs, d_rec, thr, ratio, rot, stream)
                tag = (e["name"], levelsup, voc.groups, si, rs["world"], rs["cap"])
                om, on = records_bow_oracle(t, levelsup, rs, thr, ratio, rot)
                assert np.array_equal(gm, om) and np.array_equal(gn, on), tag
                assert (gm[rs["rank"]] == -1).all() and gn[rs["rank"]] == 0, tag
                if not rs["big"]:
                    pm, pn = ref_bow.records_bow_match(t, levelsup, rs["frames"], rs["rank"], rs["cap"], thr, ratio, rot)
                    assert np.array_equal(gm, pm) and np.array_equal(gn, pn), tag + ("numpy reference",)
                total += int(gn.sum())
                d_rec.free()
    assert total > 1000


def test_records_refusals(matcher, edge_trees):
    """cap above 65 535 or below 1, a misaligned record base, a stride below hs_record_bytes(cap) or not a multiple of 4, rank outside the world"""
    ex = matcher._ex
    voc = next(iter(edge_trees[0][1].values()))
    rs = list(scenes.record_edge_sets(1))[4]
    d_rec = hipmem.DevBuf.from_numpy(rs["buf"])
    world, cap, stride, rank = rs["world"], rs["cap"], rs["stride"], rs["rank"]
    outs = [hipmem.DevBuf(world * cap * 4) for _ in range(3)]
    V = C.c_void_p
    bad = [dict(cap=65536), dict(cap=0), dict(base=d_rec.ptr + 4), dict(stride=stride - 16), dict(stride=stride + 2), dict(rank=world), dict(rank=-1),
           dict(world=0), dict(base=0)]
    for b in bad:
        a = dict(base=d_rec.ptr, stride=stride, world=world, rank=rank, cap=cap); a.update(b)
        st = ex._lib.hs_records_bow_match_device(ex._h, voc._v, V(a["base"]), a["stride"], a["world"], a["rank"], a["cap"], 50.0, 0.8, 1,
                                                 V(outs[0].ptr), V(outs[1].ptr), None)
        assert st == N.HS_ERR_INVALID, b
        st = ex._lib.hs_records_knn2_device(ex._h, V(a["base"]), a["stride"], a["world"], a["rank"], a["cap"], V(outs[0].ptr), V(outs[1].ptr), V(outs[2].ptr), None)
        assert st == N.HS_ERR_INVALID, b
    assert ex._lib.hs_records_bow_match_device(ex._h, voc._v, V(d_rec.ptr), stride, world, rank, cap, 50.0, 0.8, 1, None, V(outs[1].ptr), None) == N.HS_ERR_INVALID
    assert ex._lib.hs_bow_transform_device(ex._h, voc._v, V(d_rec.ptr), None, -1, V(outs[0].ptr), V(outs[1].ptr), V(outs[2].ptr), None) == N.HS_ERR_INVALID
    assert ex._lib.hs_bow_transform_device(ex._h, voc._v, None, None, 5, V(outs[0].ptr), V(outs[1].ptr), V(outs[2].ptr), None) == N.HS_ERR_INVALID
    assert ex._lib.hs_hamming_knn2_device(ex._h, None, 3, V(d_rec.ptr), 3, V(outs[0].ptr), V(outs[1].ptr), V(outs[2].ptr), None) == N.HS_ERR_INVALID
    assert ex._lib.hs_hamming_knn2(ex._h, None, -1, None, 0, None, None, None) == N.HS_ERR_INVALID


# ---------------------------------------------------------------- brute-force 2-NN
def test_knn2_edge_cases_all_entry_points(matcher):
    """hs_hamming_knn2 and hs_hamming_knn2_device (caller stream) on every 2-NN case; output beyond nq untouched"""
    ex = matcher._ex
    stream = hipmem.Stream()
    for seed in range(3):
        for c in scenes.knn2_edge_cases(seed):
            q, t = c["q"], c["t"]
            nq, nt = len(q), len(t)
            o = oracle.hamming_knn2(q, t)
            r = ref_bow.hamming_knn2(q, t)
            g = matcher.HammingKnn2(q, t)
            for a, b, d in zip(g, o, r):
                assert np.array_equal(a, b) and np.array_equal(a, d), (c["kind"], nq, nt)
            pad = 7
            d_q, d_t = hipmem.DevBuf.from_numpy(q), hipmem.DevBuf.from_numpy(t)
            outs = [hipmem.DevBuf((nq + pad) * 4, zero=False) for _ in range(3)]
            for b in outs:
                b.fill(0x5A)
            N.check(ex._h, ex._lib.hs_hamming_knn2_device(ex._h, C.c_void_p(d_q.ptr), nq, C.c_void_p(d_t.ptr), nt, C.c_void_p(outs[0].ptr),
                                                          C.c_void_p(outs[1].ptr), C.c_void_p(outs[2].ptr), C.c_void_p(stream.ptr)))
            stream.synchronize()
            for b, want in zip(outs, o):
                got = b.to_numpy(np.int32, nq + pad)
                assert np.array_equal(got[:nq], want) and (got[nq:] == PATTERN).all(), (c["kind"], nq, nt, "device")


def test_records_knn2_on_record_sets(matcher):
    """hs_records_knn2_device on every record set: per peer the 2-NN of the rank's descriptors over the peer's, counts clamped on the device; the
    `rank` row and the entries beyond the query count stay untouched"""
    ex = matcher._ex
    stream = hipmem.Stream()
    sets = list(scenes.record_edge_sets(9))
    for si in RECORD_ORDER:
        rs = sets[si]
        world, cap, rank = rs["world"], rs["cap"], rs["rank"]
        d_rec = hipmem.DevBuf.from_numpy(rs["buf"])
        outs = [hipmem.DevBuf(world * cap * 4, zero=False) for _ in range(3)]
        for b in outs:
            b.fill(0x5A)
        N.check(ex._h, ex._lib.hs_records_knn2_device(ex._h, C.c_void_p(d_rec.ptr), rs["stride"], world, rank, cap, C.c_void_p(outs[0].ptr),
                                                      C.c_void_p(outs[1].ptr), C.c_void_p(outs[2].ptr), C.c_void_p(stream.ptr)))
        stream.synchronize()
        got = [b.to_numpy(np.int32, world * cap).reshape(world, cap) for b in outs]
        q = rs["frames"][rank][1]
        for peer in range(world):
            if peer == rank:
                assert all((g[peer] == PATTERN).all() for g in got), (si, "rank row")
                continue
            o = oracle.hamming_knn2(q, rs["frames"][peer][1])
            for g, want in zip(got, o):
                assert np.array_equal(g[peer, :len(q)], want) and (g[peer, len(q):] == PATTERN).all(), (si, peer)
            if not rs["big"]:
                for g, want in zip(got, ref_bow.hamming_knn2(q, rs["frames"][peer][1])):
                    assert np.array_equal(g[peer, :len(q)], want), (si, peer, "numpy reference")


def test_records_knn2_on_knn2_edge_cases(matcher):
    """hs_records_knn2_device on the 2-NN cases themselves: q and t of every case packed as records 0 and 1 of a world of two (cap = max(nq, nt, 1)),
    so identical train sets, one distance, the complement, duplicates in one lane and in different lanes and the sizes around 64 and 128 reach
    k_knn2_records; both directions (rank 0 and rank 1).  Against the oracle and the numpy reference; everything else keeps the pattern."""
    ex = matcher._ex
    stream = hipmem.Stream()
    for seed in range(3):
        for c in scenes.knn2_edge_cases(seed):
            sides = (c["q"], c["t"])
            cap = max(len(c["q"]), len(c["t"]), 1)
            stride = record_bytes(cap)
            buf = np.concatenate([pack_record(scenes.plain_kps(len(d)), d, cap) for d in sides])
            d_rec = hipmem.DevBuf.from_numpy(buf)
            for rank in (0, 1):
                q, t = sides[rank], sides[1 - rank]
                outs = [hipmem.DevBuf(2 * cap * 4, zero=False) for _ in range(3)]
                for b in outs:
                    b.fill(0x5A)
                N.check(ex._h, ex._lib.hs_records_knn2_device(ex._h, C.c_void_p(d_rec.ptr), stride, 2, rank, cap, C.c_void_p(outs[0].ptr),
                                                              C.c_void_p(outs[1].ptr), C.c_void_p(outs[2].ptr), C.c_void_p(stream.ptr)))
                stream.synchronize()
                got = [b.to_numpy(np.int32, 2 * cap).reshape(2, cap) for b in outs]
                tag = (c["kind"], len(q), len(t), rank)
                for g, want, ref in zip(got, oracle.hamming_knn2(q, t), ref_bow.hamming_knn2(q, t)):
                    assert np.array_equal(g[1 - rank, :len(q)], want) and np.array_equal(want, ref), tag
                    assert (g[1 - rank, len(q):] == PATTERN).all() and (g[rank] == PATTERN).all(), tag + ("untouched",)
