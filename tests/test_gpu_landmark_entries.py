"""GPU: hs_landmark_update_entries(_device) — MapPointDBEntry::_updateEntry_ (src/core/MapPointDB.cpp:223-310) for a batch — bit-exact (a NaN only
has to meet a NaN) against the restatement in tests/ref_landmark_entry.py (pinned by tests/test_landmark_entry_ref.py), through the C
ABI, the Python methods, the scatter into device hs_landmark records and the C++ adaptor hyslam_amd/host/HipLandmarkEntries.h; and end to end:
entries updated on the device, then hs_search_by_projection_device on the refreshed records, against the host path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hipmem
import ref_landmark_entry as R
from landmark_entry_cases import KNOWN_ENTRIES, random_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
EXE = os.path.join(BUILD, "test_landmark_entries_adaptor")
KEYS = ("normal", "min_dist", "max_dist", "mean_dist", "size", "best", "median", "flags")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(gpu):
    import hyslam_amd as HS
    return HS.FeatureMatcher(extractor=HS.ORBExtractor(device=0))


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def desc_csr(descs):
    off = np.zeros(len(descs) + 1, np.int64)
    np.cumsum([len(d) for d in descs], out=off[1:])
    flat = np.concatenate([np.asarray(d, np.uint8).reshape(-1, 32) for d in descs]) if descs else np.zeros((0, 32), np.uint8)
    return off, np.ascontiguousarray(flat)


def assert_same(got, want, tag=""):
    for k in KEYS:
        if not R.same(got[k], want[k]):
            g, w = np.asarray(got[k]), np.asarray(want[k])
            bad = np.nonzero(~np.all(((g == w) | (np.isnan(g) & np.isnan(w))) if g.dtype.kind == "f" else (g == w), axis=tuple(range(1, g.ndim))))[0]
            pytest.fail("%s %s differs at %s: got %s want %s" % (tag, k, bad[:5].tolist(), g[bad[:5]].tolist(), w[bad[:5]].tolist()))


def known_batch():
    from landmark_entry_cases import ENTRY_DTYPE
    names = sorted(KNOWN_ENTRIES)
    cs = [KNOWN_ENTRIES[k] for k in names]
    ent = np.zeros(len(cs), ENTRY_DTYPE)
    ent["pos"] = [c["pos"] for c in cs]
    ent["ref_Ow"] = [c["ref_Ow"] for c in cs]
    return names, ent, [c["obs"] for c in cs], [c["descs"] for c in cs]


def test_known_answers(matcher):
    names, ent, obs, descs = known_batch()
    got = matcher.UpdateLandmarkEntries(ent, observations=obs, descriptors=descs)
    want = R.update_entries(ent, [list(o) for o in obs], descs)
    assert_same(got, want)
    for i, k in enumerate(names):                                          # and the hand-derived values themselves
        for key, v in KNOWN_ENTRIES[k]["expect"].items():
            if v is None:
                assert not got["flags"][i] & (R.HS_LM_SET_NORMAL_DEPTH if key in ("normal", "min_dist", "max_dist") else R.HS_LM_SET_MEAN), (k, key)
            else:
                assert R.same(np.asarray(got[key][i], np.asarray(got[key]).dtype), np.asarray(v, np.asarray(got[key]).dtype)), (k, key, got[key][i], v)


def test_known_answers_across_the_chunk_boundary(matcher):
    """each known landmark's observations repeated past 64 and 128: the running sums carry from one 64-observation chunk to the next"""
    names, ent, obs, descs = known_batch()
    for reps in (65, 130):
        obs_r = [np.concatenate([o] * (reps // max(len(o), 1) + 1))[:reps] if len(o) else o for o in obs]
        got = matcher.UpdateLandmarkEntries(ent, observations=obs_r, descriptors=descs)
        off = np.zeros(len(obs_r) + 1, np.int64)
        np.cumsum([len(o) for o in obs_r], out=off[1:])
        assert_same(got, R.update_entries_fast(ent, off, np.concatenate(obs_r), descs), reps)
        assert_same(got, R.update_entries(ent, [list(o) for o in obs_r], descs), reps)


@pytest.mark.parametrize("seed", [0, 1])
def test_random_ragged_batches(matcher, seed):
    ent, off, ob, descs = random_batch(seed, 20000, n_max=40, big=[(5, 5000), (777, 64), (778, 65), (9000, 128), (19999, 700)])
    got = matcher.UpdateLandmarkEntries(ent, obs_offsets=off, obs=ob, descriptors=descs)
    assert_same(got, R.update_entries_fast(ent, off, ob, descs), seed)


def test_empty_batch(matcher):
    from landmark_entry_cases import ENTRY_DTYPE, OBS_DTYPE
    got = matcher.UpdateLandmarkEntries(np.zeros(0, ENTRY_DTYPE), observations=[], descriptors=[])
    assert all(len(got[k]) == 0 for k in KEYS)
    got = matcher.UpdateLandmarkEntries(np.zeros(0, ENTRY_DTYPE), obs_offsets=np.zeros(1, np.int64), obs=np.zeros(0, OBS_DTYPE),
                                        desc_offsets=np.zeros(1, np.int64), desc=np.zeros((0, 32), np.uint8))
    assert all(len(got[k]) == 0 for k in KEYS)


def test_host_entry_point_leaves_unset_outputs_alone(matcher):
    """N = 0: the C entry point does not touch normal, min / max distance and mean distance; bad offsets are refused"""
    from hyslam_amd import _native as N
    ex = matcher._ex
    ent, off, ob, descs = random_batch(3, 300, n_max=6)
    doff, dflat = desc_csr(descs)
    L = len(ent)
    outs = [np.full((L, 3), 7.5, np.float32)] + [np.full(L, 7.5, np.float32) for _ in range(4)] + [np.full(L, 99, np.int32) for _ in range(3)]
    prm = N.LmEntryParams()
    assert ex._lib.hs_landmark_update_entries(ex._h, C.byref(prm), L, p(ent), p(off), p(ob), p(doff), p(dflat), *[p(o) for o in outs]) == N.HS_OK
    want = R.update_entries_fast(ent, off, ob, descs)
    empty = np.diff(off) == 0
    assert empty.any()
    for o, k in zip(outs, KEYS):
        w = want[k].copy()
        if k in ("normal", "min_dist", "max_dist", "mean_dist"):
            w[empty] = 7.5
        assert R.same(o, w), k
    bad = off.copy(); bad[5] = bad[6] + 1
    assert ex._lib.hs_landmark_update_entries(ex._h, C.byref(prm), L, p(ent), p(bad), p(ob), p(doff), p(dflat), *[p(o) for o in outs]) == N.HS_ERR_INVALID
    assert ex._lib.hs_landmark_update_entries(ex._h, C.byref(prm), 0, None, None, None, None, None, *([None] * 8)) == N.HS_OK


def test_host_entry_point_reuses_its_handle_across_sizes(matcher):
    for seed, L in ((20, 6000), (21, 5), (22, 15000)):
        ent, off, ob, descs = random_batch(seed, L, big=[(1, 300)])
        got = matcher.UpdateLandmarkEntries(ent, obs_offsets=off, obs=ob, descriptors=descs)
        assert_same(got, R.update_entries_fast(ent, off, ob, descs), (seed, L))


def test_parameters_are_the_factors(matcher):
    ent, off, ob, descs = random_batch(4, 500)
    got = matcher.UpdateLandmarkEntries(ent, obs_offsets=off, obs=ob, descriptors=descs, max_dist_factor=1.7, min_dist_factor=0.3)
    assert_same(got, R.update_entries_fast(ent, off, ob, descs, max_factor=1.7, min_factor=0.3))


def test_device_entry_point_scatters_into_landmark_records(matcher):
    """device pointers on a caller stream; the scatter through a permuted index map (some -1, some past the end) writes normal, min / max
    distance, size and desc of the named records only, and nothing else"""
    from hyslam_amd import _native as N
    ex = matcher._ex
    s = hipmem.Stream()
    for seed, L in ((30, 3000), (31, 9), (32, 0)):
        ent, off, ob, descs = random_batch(seed, L, big=[(1, 200)] if L > 1 else [])
        rng = np.random.default_rng(seed)
        n_lms = L + 37
        lms = np.frombuffer(rng.integers(0, 256, n_lms * N.LM_DTYPE.itemsize, dtype=np.uint8).tobytes(), N.LM_DTYPE).copy()
        index = rng.permutation(n_lms)[:L].astype(np.int32)
        if L > 4:
            index[:2] = -1
            index[2] = n_lms + 5                                          # out of range: skipped
        doff, dflat = desc_csr(descs)
        ins = [hipmem.DevBuf.from_numpy(np.ascontiguousarray(a)) if a.nbytes else hipmem.DevBuf(64) for a in (ent, off, ob, doff, dflat)]
        outs = [hipmem.DevBuf(max(L, 1) * 12)] + [hipmem.DevBuf(max(L, 1) * 4) for _ in range(7)]
        for o in outs:
            o.fill(0x55)
        d_lms, d_idx = hipmem.DevBuf.from_numpy(lms), hipmem.DevBuf.from_numpy(index if L else np.zeros(1, np.int32))
        ex.landmark_update_entries_device(L, *[b.ptr for b in ins], *[o.ptr for o in outs], d_lms=d_lms.ptr, d_lm_index=d_idx.ptr, n_lms=n_lms,
                                          stream=s.ptr)
        s.synchronize()
        got_lms = d_lms.to_numpy(N.LM_DTYPE, n_lms)
        if L == 0:
            assert outs[0].to_numpy(np.uint32, 1)[0] == 0x55555555 and got_lms.tobytes() == lms.tobytes()
            continue
        want = R.update_entries_fast(ent, off, ob, descs)
        got = {k: o.to_numpy(np.float32 if i < 5 else np.int32, L * (3 if i == 0 else 1)) for i, (k, o) in enumerate(zip(KEYS, outs))}
        got["normal"] = got["normal"].reshape(L, 3)
        empty = np.diff(off) == 0
        for k in ("normal", "min_dist", "max_dist", "mean_dist"):                 # unset outputs: device memory untouched
            assert (got[k][empty].view(np.uint32) == 0x55555555).all(), k
            got[k][empty] = np.nan
        assert_same(got, want, (seed, L))
        exp = lms.copy()
        for i in range(L):
            t = index[i]
            if t < 0 or t >= n_lms:
                continue
            if want["flags"][i] & R.HS_LM_SET_NORMAL_DEPTH:
                exp["normal"][t], exp["min_dist"][t], exp["max_dist"][t] = want["normal"][i], want["min_dist"][i], want["max_dist"][i]
            exp["size"][t] = want["size"][i]
            if want["best"][i] >= 0:
                exp["desc"][t] = descs[i][want["best"][i]]
        gb, eb = got_lms.view(np.uint8).reshape(n_lms, -1), exp.view(np.uint8).reshape(n_lms, -1)
        # NaN results may differ in sign / payload: compare them as "NaN" and everything else byte for byte
        for f in ("normal", "min_dist", "max_dist", "size"):
            nan = np.isnan(exp[f])
            assert np.array_equal(np.isnan(got_lms[f]), nan), f
            got_lms[f][nan] = exp[f][nan]
        assert got_lms.tobytes() == exp.tobytes(), np.nonzero((gb != eb).any(1))[0][:5]


def test_device_entry_point_on_the_handle_stream_and_refusals(matcher):
    from hyslam_amd import _native as N
    ex = matcher._ex
    ent, off, ob, descs = random_batch(34, 700, big=[(2, 90)])
    doff, dflat = desc_csr(descs)
    L = len(ent)
    ins = [hipmem.DevBuf.from_numpy(np.ascontiguousarray(a)) for a in (ent, off, ob, doff, dflat)]
    outs = [hipmem.DevBuf(L * 12)] + [hipmem.DevBuf(L * 4) for _ in range(7)]
    ex.landmark_update_entries_device(L, *[b.ptr for b in ins], *[o.ptr for o in outs])
    ex.synchronize()
    want = R.update_entries_fast(ent, off, ob, descs)
    assert R.same(outs[4].to_numpy(np.float32, L), want["size"]) and np.array_equal(outs[5].to_numpy(np.int32, L), want["best"])
    prm = N.LmEntryParams()
    args = [b.ptr for b in ins]
    args[4] += 4                                                                  # misaligned descriptors
    assert ex._lib.hs_landmark_update_entries_device(ex._h, C.byref(prm), L, *args, *[o.ptr for o in outs], None, None, 0, None) == N.HS_ERR_INVALID
    # d_lms without an index map
    assert ex._lib.hs_landmark_update_entries_device(ex._h, C.byref(prm), L, *[b.ptr for b in ins], *[o.ptr for o in outs], outs[0].ptr, None, 1,
                                                     None) == N.HS_ERR_INVALID


def _build_adaptor():
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread",
                           os.path.join(ROOT, "tests", "cpp", "test_landmark_entries_adaptor.cpp"), "-o", EXE,
                           "-L" + os.path.join(ROOT, "hyslam_amd"), "-lhyslam_amd", "-Wl,-rpath," + os.path.join(ROOT, "hyslam_amd")])


def test_cpp_adaptor(tmp_path):
    ent, off, ob, descs = random_batch(40, 2500, big=[(0, 66), (1200, 300)])
    doff, dflat = desc_csr(descs)
    L = len(ent)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.int32(L).tobytes() + ent.tobytes() + off.tobytes() + ob.tobytes() + doff.tobytes() + dflat.tobytes())
    _build_adaptor()
    r = subprocess.run([EXE, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"LANDMARK ENTRIES ADAPTOR OK" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    rec = np.dtype([("normal", "<f4", 3), ("min_dist", "<f4"), ("max_dist", "<f4"), ("mean_dist", "<f4"), ("size", "<f4"), ("best", "<i4"),
                    ("median", "<i4"), ("flags", "<i4")])
    got = raw.view(rec)
    assert len(got) == 2 * L
    want = R.update_entries_fast(ent, off, ob, descs)
    for half in (got[:L], got[L:]):                                               # the calling thread's handle, then an explicit one
        g = {k: half[k].copy() for k in KEYS}
        for k in ("normal", "min_dist", "max_dist", "mean_dist"):
            unset = (g["flags"] & (R.HS_LM_SET_MEAN if k == "mean_dist" else R.HS_LM_SET_NORMAL_DEPTH)) == 0
            g[k][unset] = np.nan
        assert_same(g, want)


def test_end_to_end_device_update_then_projection_search(matcher):
    """BA moved the points -> entries updated on the device, scattered into the resident hs_landmark array -> hs_search_by_projection_device.
    Host path: the restated entries written into the same records -> hs_search_by_projection.  The matches must be identical."""
    import oracle
    import scenes
    from hyslam_amd import _native as N
    ex = matcher._ex
    sc = scenes.projection_scene(5)
    fa = sc["frame_args"]
    lms = np.ascontiguousarray(sc["lms"], N.LM_DTYPE)
    L = len(lms)
    rng = np.random.default_rng(5)
    Fh, keep = oracle.make_frame_view(N.FrameView, **fa)
    Ow0 = np.array(Fh.Ow[:], np.float32)
    # observations: 1..8 key frames around the frame's camera centre, the keypoint sizes of the frame's own scale levels
    n = rng.integers(0, 9, L)
    off = np.zeros(L + 1, np.int64)
    np.cumsum(n, out=off[1:])
    owner = np.repeat(np.arange(L), n)
    from landmark_entry_cases import ENTRY_DTYPE, OBS_DTYPE
    ob = np.zeros(int(off[-1]), OBS_DTYPE)
    ob["Ow"] = (Ow0 + rng.normal(0, 0.3, (len(ob), 3))).astype(np.float32)
    ob["fx"], ob["fy"], ob["cx"], ob["cy"] = fa["fx"], fa["fy"], fa["cx"], fa["cy"]
    ob["u"], ob["v"] = rng.uniform(0, 640, len(ob)), rng.uniform(0, 480, len(ob))
    ob["kp_size"] = (31.0 * 1.2 ** rng.integers(0, 8, len(ob))).astype(np.float32)
    ob["assoc_pos"] = lms["pos"][owner]
    ob["assoc"] = (rng.random(len(ob)) > 0.05).astype(np.int32)
    ent = np.zeros(L, ENTRY_DTYPE)
    ent["pos"] = lms["pos"]
    ent["ref_Ow"] = np.where(n[:, None] > 0, ob["Ow"][np.minimum(off[:-1], max(len(ob) - 1, 0))] if len(ob) else Ow0, Ow0)
    descs = []
    for i in range(L):
        k = int(rng.integers(0, 5))
        d = np.repeat(lms["desc"][i][None], k, 0)
        d ^= (rng.random(d.shape) < 0.03).astype(np.uint8) * np.uint8(1 << int(rng.integers(0, 8)))
        descs.append(d)
    # host path
    want = R.update_entries_fast(ent, off, ob, descs)
    host = lms.copy()
    set_nd = (want["flags"] & R.HS_LM_SET_NORMAL_DEPTH) != 0
    host["normal"][set_nd], host["min_dist"][set_nd], host["max_dist"][set_nd] = want["normal"][set_nd], want["min_dist"][set_nd], want["max_dist"][set_nd]
    host["size"] = want["size"]
    for i in np.nonzero(want["best"] >= 0)[0]:
        host["desc"][i] = descs[i][want["best"][i]]
    pp = N.ProjParams(3.0, matcher.TH_HIGH, matcher.mfNNratio, 0.5, 1.5, 1, 1, 0)
    hi, hd, hn = np.full(L, -1, np.int32), np.full(L, -1, np.float32), C.c_int32()
    N.check(ex._h, ex._lib.hs_search_by_projection(ex._h, C.byref(Fh), p(host), L, C.byref(pp), p(hi), p(hd), C.byref(hn)))
    assert hn.value > 50
    # device path: the frame and the (stale) landmark records resident, entries updated and scattered in place, then the search
    s = hipmem.Stream()
    Fd, keep2 = oracle.make_frame_view(N.FrameView, **fa)
    fb = [hipmem.DevBuf.from_numpy(np.ascontiguousarray(a)) for a in (fa["kps"], fa["desc"], fa["uR"], fa["kp_lm_obs"])]
    Fd.kps, Fd.desc, Fd.uR, Fd.kp_lm_obs = fb[0].ptr, fb[1].ptr, fb[2].ptr, fb[3].ptr
    doff, dflat = desc_csr(descs)
    ins = [hipmem.DevBuf.from_numpy(np.ascontiguousarray(a)) for a in (ent, off, ob, doff, dflat)]
    outs = [hipmem.DevBuf(L * 12)] + [hipmem.DevBuf(L * 4) for _ in range(7)]
    d_lms, d_idx = hipmem.DevBuf.from_numpy(lms), hipmem.DevBuf.from_numpy(np.arange(L, dtype=np.int32))
    ex.landmark_update_entries_device(L, *[b.ptr for b in ins], *[o.ptr for o in outs], d_lms=d_lms.ptr, d_lm_index=d_idx.ptr, n_lms=L, stream=s.ptr)
    d_i, d_d, d_n = hipmem.DevBuf(L * 4), hipmem.DevBuf(L * 4), hipmem.DevBuf(4)
    N.check(ex._h, ex._lib.hs_search_by_projection_device(ex._h, C.byref(Fd), C.c_void_p(d_lms.ptr), L, C.byref(pp), C.c_void_p(d_i.ptr),
                                                          C.c_void_p(d_d.ptr), C.c_void_p(d_n.ptr), C.c_void_p(s.ptr)))
    s.synchronize()
    assert np.array_equal(d_i.to_numpy(np.int32, L), hi)
    assert np.array_equal(d_d.to_numpy(np.float32, L), hd)
    assert int(d_n.to_numpy(np.int32, 1)[0]) == hn.value
    # the refresh changed what the search sees: the stale records match differently
    si, sd, sn = np.full(L, -1, np.int32), np.full(L, -1, np.float32), C.c_int32()
    N.check(ex._h, ex._lib.hs_search_by_projection(ex._h, C.byref(Fh), p(lms), L, C.byref(pp), p(si), p(sd), C.byref(sn)))
    assert not np.array_equal(si, hi)
