"""GPU: hs_kf_votes(_device) and hs_kf_redundancy(_device) — CovisNode::UpdateConnections, TrackLocalMap::UpdateLocalKeyFrames and KeyFrameCuller::run
over one observation table — against the restatement in tests/ref_kfgraph.py (pinned by tests/test_kfgraph_ref.py).  Integer results: EVERY output is
compared exactly.  Through the C ABI, the Python methods, the device forms on a caller stream, the C++ adaptor hyslam_amd/host/HipKeyFrameGraph.h, and
end to end: the ordered rows of a whole-graph recompute handed to hs_place_query_reloc_device as its neighbour table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hipmem
import ref_kfgraph as R
from kfgraph_cases import (KNOWN_REDUNDANCY, KNOWN_REDUNDANCY_TABLE, KNOWN_VOTES, csr, key_frame_queries, random_candidates, random_table, table)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
EXE = os.path.join(BUILD, "test_kfgraph_adaptor")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(gpu):
    import hyslam_amd as HS
    return HS.FeatureMatcher(extractor=HS.ORBExtractor(device=0))


@pytest.fixture(scope="module")
def graph():
    """64 key frames, 3 000 landmarks with up to 40 observations (one with all 64), the whole-graph queries and their reference — computed once"""
    T = random_table(7, 64, 3000, max_obs=40, big=[(11, 64)])
    off, q_lm, ids = key_frame_queries(T)
    return T, off, q_lm, ids, R.votes_fast(T, off, q_lm, ids, 0, 15, 10)


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def assert_votes(got, want, tag=""):
    k = R.same(got, want, R.VOTE_KEYS)
    if k is not None:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        bad = np.argwhere(g != w)[:5]
        pytest.fail("%s %s differs at %s: got %s want %s" % (tag, k, bad.tolist(), [g[tuple(b)] for b in bad], [w[tuple(b)] for b in bad]))


def assert_red(got, want, tag=""):
    k = R.same(got, want, R.RED_KEYS)
    assert k is None, (tag, k, np.asarray(got[k])[:8], np.asarray(want[k])[:8])


def native_table(N, T, dev=False):
    order = ("lm_obs_offsets", "lm_obs_kf", "lm_obs_octave", "lm_bad", "lm_nobs", "kf_bad", "kf_id")
    if dev:
        keep = [hipmem.DevBuf.from_numpy(T[k]) for k in order]
        return N.KfTable(len(T["lm_bad"]), len(T["kf_id"]), *[b.ptr for b in keep]), keep
    keep = [np.ascontiguousarray(T[k]) for k in order]
    return N.KfTable(len(T["lm_bad"]), len(T["kf_id"]), *[a.ctypes.data for a in keep]), keep


def c_votes(matcher, T, off, q_lm, ids, count_bad_kf, th, cap, weights=True, fill=None):
    from hyslam_amd import _native as N
    ex = matcher._ex
    KT, keep = native_table(N, T)
    Q, n_kf = len(off) - 1, len(T["kf_id"])
    v = 0 if fill is None else fill
    out = dict(weights=np.full((Q, n_kf), v, np.int32) if weights else None, max_slot=np.full(Q, v, np.int32), max_count=np.full(Q, v, np.int32),
               ordered_slot=np.full((Q, cap), v, np.int32), ordered_weight=np.full((Q, cap), v, np.int32), n_ordered=np.full(Q, v, np.int32))
    q_lm, off = np.ascontiguousarray(q_lm, np.int32), np.ascontiguousarray(off, np.int64)
    ids = None if ids is None else np.ascontiguousarray(ids, np.int64)
    st = ex._lib.hs_kf_votes(ex._h, C.byref(KT), Q, p(off), p(q_lm), p(ids), count_bad_kf, th, p(out["weights"]), p(out["max_slot"]),
                             p(out["max_count"]), p(out["ordered_slot"]), p(out["ordered_weight"]), cap, p(out["n_ordered"]))
    return st, out


# ---- known answers
@pytest.mark.parametrize("name", sorted(KNOWN_VOTES))
def test_known_votes(matcher, name):
    from hyslam_amd import _native as N
    c = KNOWN_VOTES[name]
    got = matcher.KeyFrameVotes(c["T"], queries=c["queries"], self_id=c["self_id"], count_bad_kf=c["count_bad_kf"], th=c["th"], cap=c["cap"])
    off, q_lm = csr(c["queries"])
    st, got_c = c_votes(matcher, c["T"], off, q_lm, c["self_id"], c["count_bad_kf"], c["th"], c["cap"], fill=77)
    assert st == N.HS_OK
    for k in R.VOTE_KEYS:
        assert np.array_equal(got[k], np.asarray(c[k])), (name, k, got[k])
        assert np.array_equal(got_c[k], np.asarray(c[k])), (name, "C ABI", k, got_c[k])


@pytest.mark.parametrize("name", sorted(KNOWN_REDUNDANCY))
def test_known_redundancy(matcher, name):
    c = KNOWN_REDUNDANCY[name]
    got = matcher.KeyFrameRedundancy(KNOWN_REDUNDANCY_TABLE, c["cand_slot"], c["cand_th_depth"], items=c["items"], is_mono=c["is_mono"],
                                     th_obs=c["th_obs"], frac_redundant=c["frac"])
    for k in R.RED_KEYS:
        assert np.array_equal(got[k], np.asarray(c[k])), (name, k, got[k])


# ---- random ragged batches
def test_whole_graph_recompute(matcher, graph):
    T, off, q_lm, ids, want = graph
    got = matcher.KeyFrameVotes(T, q_offsets=off, q_lm=q_lm, self_id=ids, th=15, cap=10)
    assert_votes(got, want)
    assert want["n_ordered"].min() > 10                                                   # every row truncated at cap = 10 ...
    got = matcher.KeyFrameVotes(T, q_offsets=off, q_lm=q_lm, self_id=ids, th=15, cap=64, weights=False)
    assert got["weights"] is None and got["n_ordered"].max() < 64                         # ... and padded at cap = 64
    assert_votes(got, R.votes_fast(T, off, q_lm, ids, 0, 15, 64))


@pytest.mark.parametrize("count_bad_kf", [0, 1])
def test_frame_shaped_queries(matcher, graph, count_bad_kf):
    """queries of 2 000 landmarks, none, and one that lists its landmarks twice; nothing excluded, as UpdateLocalKeyFrames"""
    T = graph[0]
    rng = np.random.default_rng(3)
    dup = rng.integers(0, 3000, 300)
    queries = [rng.choice(3000, 2000, replace=False), [], rng.choice(3000, 2000, replace=False), np.concatenate([dup, dup]), [5]]
    got = matcher.KeyFrameVotes(T, queries=queries, count_bad_kf=count_bad_kf, th=15, cap=64)
    off, q_lm = csr(queries)
    want = R.votes_fast(T, off, q_lm, None, count_bad_kf, 15, 64)
    assert_votes(got, want, count_bad_kf)
    assert want["n_ordered"][1] == 0 and want["max_slot"][1] == -1
    once = R.votes_fast(T, *csr([dup]), None, count_bad_kf, 15, 64)
    assert np.array_equal(got["weights"][3], 2 * once["weights"][0])
    if count_bad_kf:
        assert (got["weights"][0][T["kf_bad"] != 0] > 0).any() and not np.isin(np.nonzero(T["kf_bad"])[0], got["ordered_slot"][0]).any()


def test_the_lds_limit(matcher):
    """n_kf one below, at and one above HS_KF_LDS_SLOTS: LDS counters, then the global rows with device atomics; tiny lists"""
    from hyslam_amd import _native as N
    lim = N.HS_KF_LDS_SLOTS
    for n_kf in (lim - 1, lim, lim + 1):
        T = random_table(n_kf, n_kf, 60, max_obs=30, big=[(0, 500)])
        T["lm_obs_kf"][int(T["lm_obs_offsets"][1]) - 1] = n_kf - 1                     # the last slot is used (landmark 0 stays ascending)
        queries = [np.arange(60), [0, 1, 2], [], np.arange(60).repeat(2)]
        off, q_lm = csr(queries)
        ids = np.array([-1, int(T["kf_id"][T["lm_obs_kf"][0]]), -1, -1], np.int64)
        for count_bad_kf, th, cap, weights in ((0, 2, 16, True), (1, 1, 700, True), (0, 1, 16, False)):
            st, got = c_votes(matcher, T, off, q_lm, ids, count_bad_kf, th, cap, weights=weights)
            assert st == N.HS_OK
            assert_votes(got, R.votes_fast(T, off, q_lm, ids, count_bad_kf, th, cap), (n_kf, count_bad_kf, th, cap))


@pytest.mark.parametrize("n_kf", [12, 2000])
def test_ordered_list_lengths(matcher, n_kf):
    """lists of 1, 64, 65, HS_KF_SORT_PASS and HS_KF_SORT_PASS + 1 entries (the last one is ranked from the counters), with all weights equal and with
    distinct ones; cap below, at and above the length"""
    from hyslam_amd import _native as N
    one_pass = N.HS_KF_SORT_PASS
    if n_kf < 2000:
        lengths = [1, n_kf]
    else:
        lengths = [1, 64, 65, one_pass, one_pass + 1, n_kf]
    for n in lengths:
        # landmark 0 is seen by slots 0 .. n-1 (all weights equal); landmarks 1.. make the weights of every third slot differ
        obs = [list(range(n))] + [list(range(k, n, 3)) for k in range(0, min(n, 7))]
        T = table(n_kf, obs)
        for queries in ([[0]], [list(range(len(obs)))]):
            off, q_lm = csr(queries)
            for cap in sorted({max(n - 1, 1), n, n + 3, 10}):
                st, got = c_votes(matcher, T, off, q_lm, None, 0, 1, cap, fill=55)
                assert st == N.HS_OK
                want = R.votes_fast(T, off, q_lm, None, 0, 1, cap)
                assert want["n_ordered"][0] == n
                assert_votes(got, want, (n_kf, n, cap))
                if cap > n:
                    assert (got["ordered_slot"][0, n:] == -1).all() and (got["ordered_weight"][0, n:] == 0).all()

def test_redundancy_batches(matcher, graph):
    """candidates with 0, 1, 63, 64, 65 and 2 000 items, a landmark with 700 observations; mono and stereo, other thresholds"""
    T = random_table(9, 800, 3000, max_obs=40, big=[(17, 700), (18, 64), (19, 65)])
    cand = random_candidates(9, T, [0, 1, 63, 64, 65, 2000, 300])
    cand["item_lm"][70:75] = 17
    cand["item_lm"][-40:] = 17                                                         # the long list, many times in one candidate
    for is_mono, th_obs, frac in ((0, 3, 0.9), (1, 3, 0.9), (0, 5, 0.5), (1, 1, 0.05)):
        got = matcher.KeyFrameRedundancy(T, cand["cand_slot"], cand["cand_th_depth"], cand_offsets=cand["cand_offsets"], item_lm=cand["item_lm"],
                                         item_octave=cand["item_octave"], item_depth=cand["item_depth"], is_mono=is_mono, th_obs=th_obs,
                                         frac_redundant=frac)
        want = R.redundancy_fast(T, cand["cand_slot"], cand["cand_th_depth"], cand["cand_offsets"], cand["item_lm"], cand["item_octave"],
                                 cand["item_depth"], is_mono, th_obs, frac)
        assert_red(got, want, (is_mono, th_obs, frac))
        assert want["n_mps"][0] == 0 and want["n_redundant"].max() > 0
    # the list form of the Python method
    items = [np.stack([cand["item_lm"][b:e], cand["item_octave"][b:e], cand["item_depth"][b:e]], 1)
             for b, e in zip(cand["cand_offsets"][:-1], cand["cand_offsets"][1:])]
    got = matcher.KeyFrameRedundancy(T, cand["cand_slot"], cand["cand_th_depth"], items=items)
    assert_red(got, R.redundancy_fast(T, cand["cand_slot"], cand["cand_th_depth"], cand["cand_offsets"], cand["item_lm"], cand["item_octave"],
                                      cand["item_depth"]))


def test_host_forms_refuse_broken_offsets_and_leave_outputs_alone(matcher, graph):
    from hyslam_amd import _native as N
    ex = matcher._ex
    T, off, q_lm, ids, _ = graph

    def untouched(out):
        return all(v is None or (np.asarray(v) == 99).all() for v in out.values())
    broken_q = off.copy(); broken_q[5] = broken_q[6] + 1
    st, out = c_votes(matcher, T, broken_q, q_lm, ids, 0, 15, 10, fill=99)
    assert st == N.HS_ERR_INVALID and untouched(out)
    neg = off.copy(); neg[0] = -1
    st, out = c_votes(matcher, T, neg, q_lm, ids, 0, 15, 10, fill=99)
    assert st == N.HS_ERR_INVALID and untouched(out)
    T2 = dict(T); T2["lm_obs_offsets"] = T["lm_obs_offsets"].copy(); T2["lm_obs_offsets"][100] = T2["lm_obs_offsets"][101] + 2
    st, out = c_votes(matcher, T2, off, q_lm, ids, 0, 15, 10, fill=99)
    assert st == N.HS_ERR_INVALID and untouched(out)
    bad_lm = q_lm.copy(); bad_lm[3] = 3000                                             # a landmark index outside the table
    st, out = c_votes(matcher, T, off, bad_lm, ids, 0, 15, 10, fill=99)
    assert st == N.HS_ERR_INVALID and untouched(out)
    st, out = c_votes(matcher, T, off, q_lm, ids, 0, 15, 10, fill=99)
    assert st == N.HS_OK and not untouched(out)
    # redundancy
    cand = random_candidates(1, T, [5, 9, 0, 30])
    KT, keep = native_table(N, T)
    KT2, keep2 = native_table(N, T2)
    outs = [np.full(4, 99, np.int32), np.full(4, 99, np.int32), np.full(4, 99, np.uint8)]
    args = lambda kt, coff: (ex._h, C.byref(kt), 4, p(cand["cand_slot"]), p(cand["cand_th_depth"]), p(coff), p(cand["item_lm"]), p(cand["item_octave"]),
                             p(cand["item_depth"]), 0, 3, 0.9, p(outs[0]), p(outs[1]), p(outs[2]))
    broken_c = cand["cand_offsets"].copy(); broken_c[2] = broken_c[1] - 1
    assert ex._lib.hs_kf_redundancy(*args(KT, broken_c)) == N.HS_ERR_INVALID and all((o == 99).all() for o in outs)
    assert ex._lib.hs_kf_redundancy(*args(KT2, cand["cand_offsets"])) == N.HS_ERR_INVALID and all((o == 99).all() for o in outs)
    assert ex._lib.hs_kf_redundancy(*args(KT, cand["cand_offsets"])) == N.HS_OK and outs[0][2] == 0 and outs[2][2] == 0
    assert ex._lib.hs_kf_votes(ex._h, C.byref(KT), 0, None, None, None, 0, 15, None, None, None, None, None, 10, None) == N.HS_OK


def test_device_forms_on_a_stream(matcher, graph):
    """device pointers, a caller stream, sentinel-filled outputs: every entry is written (the padding too), nothing past the arrays"""
    from hyslam_amd import _native as N
    ex = matcher._ex
    T, off, q_lm, ids, want = graph
    s = hipmem.Stream()
    KT, keep = native_table(N, T, dev=True)
    Q, n_kf, cap = len(off) - 1, len(T["kf_id"]), 10
    ins = [hipmem.DevBuf.from_numpy(a) for a in (off, q_lm, ids)]
    sizes = (Q * n_kf, Q, Q, Q * cap, Q * cap, Q)
    outs = [hipmem.DevBuf((n + 8) * 4) for n in sizes]
    for o in outs:
        o.fill(0x55)
    N.check(ex._h, ex._lib.hs_kf_votes_device(ex._h, C.byref(KT), Q, ins[0].ptr, ins[1].ptr, ins[2].ptr, 0, 15, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                              outs[3].ptr, outs[4].ptr, cap, outs[5].ptr, s.ptr))
    s.synchronize()
    got = {}
    for k, o, n in zip(R.VOTE_KEYS, outs, sizes):
        a = o.to_numpy(np.int32, n + 8)
        assert (a[n:].view(np.uint32) == 0x55555555).all(), k
        got[k] = a[:n].reshape(np.asarray(want[k]).shape)
    assert_votes(got, want)
    # without the weights, on the handle's own stream
    for o in outs:
        o.fill(0x55)
    N.check(ex._h, ex._lib.hs_kf_votes_device(ex._h, C.byref(KT), Q, ins[0].ptr, ins[1].ptr, ins[2].ptr, 0, 15, None, outs[1].ptr, outs[2].ptr,
                                              outs[3].ptr, outs[4].ptr, cap, outs[5].ptr, None))
    ex.synchronize()
    assert (outs[0].to_numpy(np.uint32, 4) == 0x55555555).all()
    assert np.array_equal(outs[3].to_numpy(np.int32, Q * cap).reshape(Q, cap), want["ordered_slot"])
    # beyond the LDS limit the weights rows are the counters: required
    big = N.KfTable(KT.L, N.HS_KF_LDS_SLOTS + 1, *[b.ptr for b in keep])
    assert ex._lib.hs_kf_votes_device(ex._h, C.byref(big), Q, ins[0].ptr, ins[1].ptr, ins[2].ptr, 0, 15, None, outs[1].ptr, outs[2].ptr,
                                      outs[3].ptr, outs[4].ptr, cap, outs[5].ptr, None) == N.HS_ERR_INVALID
    # redundancy
    cand = random_candidates(2, T, [0, 64, 700, 1])
    Cn = 4
    cin = [hipmem.DevBuf.from_numpy(cand[k]) for k in ("cand_slot", "cand_th_depth", "cand_offsets", "item_lm", "item_octave", "item_depth")]
    couts = [hipmem.DevBuf(64), hipmem.DevBuf(64), hipmem.DevBuf(64)]
    for o in couts:
        o.fill(0x55)
    N.check(ex._h, ex._lib.hs_kf_redundancy_device(ex._h, C.byref(KT), Cn, *[b.ptr for b in cin], 0, 3, 0.9, *[o.ptr for o in couts], s.ptr))
    s.synchronize()
    wantr = R.redundancy_fast(T, cand["cand_slot"], cand["cand_th_depth"], cand["cand_offsets"], cand["item_lm"], cand["item_octave"], cand["item_depth"])
    gotr = dict(n_mps=couts[0].to_numpy(np.int32, Cn), n_redundant=couts[1].to_numpy(np.int32, Cn), cull=couts[2].to_numpy(np.uint8, Cn))
    assert_red(gotr, wantr)
    assert (couts[0].to_numpy(np.uint32, 16)[Cn:] == 0x55555555).all() and (couts[2].to_numpy(np.uint8, 64)[Cn:] == 0x55).all()


def test_end_to_end_ordered_rows_are_the_place_query_neighbours(matcher, graph):
    """whole-graph recompute with cap = 10 on the device -> the rows ARE d_neigh of hs_place_query_reloc_device; the candidates equal those of
    tests/ref_place.py fed with the neighbour lists of tests/ref_kfgraph.py"""
    import hyslam_amd as HS
    import ref_place
    from hyslam_amd import _native as N
    from place_cases import random_scene
    ex = matcher._ex
    T, off, q_lm, ids, want = graph
    n_kf = len(T["kf_id"])
    sc = random_scene(5, n_kf, 1000, erase=0.0)
    rec, ref = HS.PlaceRecognizer(1000, ex), ref_place.PlaceRecognizerRef(1000)
    for i, (_, w, v) in enumerate(sc["entries"]):                                      # key = slot: ascending key order is ascending slot order
        assert rec.add(i, (w, v)) == i
        ref.add(i, w, v)
    neigh = {i: [s for s, _ in want["ordered"][i][:10]] for i in range(n_kf)}
    s = hipmem.Stream()
    KT, keep = native_table(N, T, dev=True)
    ins = [hipmem.DevBuf.from_numpy(a) for a in (off, q_lm, ids)]
    d_neigh, d_w = hipmem.DevBuf(n_kf * 10 * 4), hipmem.DevBuf(n_kf * 10 * 4)
    small = [hipmem.DevBuf(n_kf * 4) for _ in range(3)]
    N.check(ex._h, ex._lib.hs_kf_votes_device(ex._h, C.byref(KT), n_kf, ins[0].ptr, ins[1].ptr, ins[2].ptr, 0, 15, None, small[0].ptr, small[1].ptr,
                                              d_neigh.ptr, d_w.ptr, 10, small[2].ptr, s.ptr))
    hits = 0
    for q in sc["queries"]:
        qw, qv = q["query"]
        d_qw, d_qv = hipmem.DevBuf.from_numpy(np.ascontiguousarray(qw, np.int32)), hipmem.DevBuf.from_numpy(np.ascontiguousarray(qv, np.float64))
        d_c, d_n = hipmem.DevBuf(n_kf * 4), hipmem.DevBuf(4)
        N.check(ex._h, ex._lib.hs_place_query_reloc_device(rec._db, d_qw.ptr, d_qv.ptr, None, len(qw), d_neigh.ptr, d_c.ptr, n_kf, d_n.ptr,
                                                           None, None, None, None, s.ptr))
        s.synchronize()
        n = int(d_n.to_numpy(np.int32, 1)[0])
        keys, _ = ref.detect_reloc(qw, qv, neigh)
        assert d_c.to_numpy(np.int32, n).tolist() == keys
        hits += len(keys) > 0
    assert hits > 0
    rec.close()


def _build_adaptor():
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread",
                           os.path.join(ROOT, "tests", "cpp", "test_kfgraph_adaptor.cpp"), "-o", EXE,
                           "-L" + os.path.join(ROOT, "hyslam_amd"), "-lhyslam_amd", "-Wl,-rpath," + os.path.join(ROOT, "hyslam_amd")])


def test_cpp_adaptor():
    """hyslam_amd/host/HipKeyFrameGraph.h on the cv_compat.h stand-ins against a std::map restatement of the three reference functions, with a culling
    sequence in which the first cull changes a later candidate's verdict"""
    _build_adaptor()
    r = subprocess.run([EXE], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"KEYFRAME GRAPH ADAPTOR OK" in r.stdout, r.stdout + r.stderr
