"""GPU: the resident chain over RUNS of frames through one set of caller-owned buffers (tests/chain_run.py; tests/test_chain_run_ref.py holds the runs'
properties on the CPU).  hs_track_frame_device, then on the same stream and for every frame the reference tracks hs_track_keyframe_device and
hs_landmark_update_entries_device, frame after frame into ONE block of device memory that holds d_work, both hs_track_state sets, every field of
hs_track_out and hs_keyframe_out, the entry update's eight outputs and the key-frame stages' work area, each at the maximum over the run with at
least 64 guard bytes behind it.  The block is filled once before the first frame and never again; every frame passes its own n, n_last, L, cap and
new_cap, so the layouts inside the work areas and the extents of the outputs move from frame to frame.

Every frame of every mode is held to two things.
 (a) the reference, as tests/test_gpu_track.py and tests/test_gpu_keyframe.py compare a single case: every integer exactly, Tcw_d within TAU;
     ref_keyframe.literal and ref_landmark_entry.update_entries from what the tracking chain left on the device.  Slot H's case is built from the
     DEVICE's outputs of G and must qualify.
 (b) the same case alone in fresh 0x55 buffers: the fields a call defines completely byte for byte; edges, flags and creation records up to the count
     the call wrote; every byte behind that count, every byte of a buffer the frame does not name and every guard byte as it was BEFORE the frame.

Modes: waited (a host wait and a read after every frame) under four fills, three of them with hs_debug_poison on; back to back on a fresh handle (no
host call that waits between the first launch and the last, snapshots by device-to-device copies on the same stream, the arena regrowing under way);
the waited run backwards and rotated; the reference-key-frame pair (hs_search_by_bow_kf_device, hs_frame_associate_views_device) waited and back to
back.  No tolerance but TAU."""
import time

import numpy as np
import pytest

import chain_run as CR
import hipmem
import ref_landmark_entry as RL
import ref_keyframe as RKF
from chain_compare import TAU, WHOLE, compare_keyframe, compare_track
from devbuf import dev, guarded, read

pytestmark = pytest.mark.gpu

GUARD = 64
FILLS = (0x55, 0x00, 0xFF, 0xA5)
STATE = ("kp_lm", "kp_outl", "n_matches", "kp_lm_obs")
KF_WHOLE = ("result", "pose_view", "obs_offsets", "desc_offsets", "lm_index")
KF_RECORDS = ("new_view", "new_pos", "entries", "obs", "desc")
EU = (12, 4, 4, 4, 4, 4, 4, 4)                                  # bytes per row of the entry update's outputs: normal, then seven 4-byte arrays
KF_RESULT_BYTES = 4 * len(RKF.RESULT_KEYS)
assert TAU == 2.1e-9


@pytest.fixture(scope="module")
def tracker(gpu):
    import hyslam_amd as HS
    return HS.FrameTracker(HS.ORBExtractor(device=0))


def up(v, a=256):
    return (v + a - 1) // a * a


# ---------------------------------------------------------------- the shared block
def track_fields(N, f):
    """(name, dtype, count) of every hs_track_out field at frame f's sizes"""
    sizes = dict(n=f.n, n_last=f.n_last, n_kf=f.n_kf, cap=f.cap)
    out = []
    for spec, prefix in ((N.TRACK_OUT_HEAD, ""), (N.LOCAL_MAP_OUT_SPEC, "local."), (N.TRACK_OUT_TAIL, "")):
        out += [(prefix + k, N.track_out_dtype(kind), sizes.get(cnt, cnt)) for k, kind, cnt in spec]
    return out


def keyframe_fields(N, new_cap):
    sizes = dict(new_cap=new_cap, new_cap1=new_cap + 1, new_cap3=3 * new_cap, new_cap32=32 * new_cap)
    return [("kf." + k, N.track_out_dtype(kind), sizes.get(cnt, cnt)) for k, kind, cnt in N.KEYFRAME_OUT_SPEC]


def state_fields(f, s):
    return [("st%d.kp_lm" % s, np.dtype(np.int32), f.n), ("st%d.kp_outl" % s, np.dtype(np.uint8), f.n), ("st%d.n_matches" % s, np.dtype(np.int32), 1),
            ("st%d.kp_lm_obs" % s, np.dtype(np.int32), f.n)]


def frame_fields(tracker, N, f):
    """everything frame f may name in the block: name -> bytes"""
    need = {k: dt.itemsize * cnt for k, dt, cnt in track_fields(N, f) + keyframe_fields(N, f.new_cap) + state_fields(f, 0) + state_fields(f, 1)}
    need.update({"eu.%d" % i: row * f.new_cap for i, row in enumerate(EU)})
    need["work"] = tracker.track_work_bytes(f.n, f.n_last, f.L, f.cap)
    need["kfwork"] = tracker.keyframe_work_bytes(f.n, f.n_kf, f.new_cap)
    return need


class Block:
    """one device allocation laid out from {field: bytes}: every field 256-byte aligned, at least GUARD bytes of the fill behind it"""

    def __init__(self, cap, fill):
        self.off, self.cap, at = {}, cap, 0
        for k in cap:
            self.off[k] = at
            at = up(at + cap[k] + GUARD)
        self.total, self.fill = at, fill
        self.buf = hipmem.DevBuf(self.total, zero=False)
        self.buf.fill(fill)
        self.pad = np.ones(self.total, bool)                     # the bytes of no field: guards
        for k in cap:
            self.pad[self.off[k]:self.off[k] + cap[k]] = False

    def ptr(self, k, byte=0):
        return self.buf.ptr + self.off[k] + byte

    def snapshot(self):
        return self.buf.to_numpy(np.uint8, self.total)


def largest(needs):
    cap = {}
    for need in needs:
        for k, b in need.items():
            cap[k] = max(cap.get(k, 16), b)
    return cap


def chain_block(tracker, N, frames, fill, state_seed):
    """the block of a run: every field at the maximum over the frames, filled once; the two state sets dirty as Chain's (the motion model clears them)"""
    blk = Block(largest(frame_fields(tracker, N, f) for f in frames), fill)
    rng = np.random.default_rng(state_seed)
    nmax = blk.cap["st0.kp_lm"] // 4
    for s in (0, 1):
        for k, a in zip(STATE, (rng.integers(-1, frames[0].L, nmax).astype(np.int32), rng.integers(0, 3, nmax).astype(np.uint8), np.array([17], np.int32),
                                rng.integers(-1, 3, nmax).astype(np.int32))):
            hipmem._ok(hipmem.hip().hipMemcpy(blk.ptr("st%d.%s" % (s, k)), a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")
    return blk


def view(snap, blk, k, dt, cnt):
    return snap[blk.off[k]:blk.off[k] + dt.itemsize * cnt].view(dt)


# ---------------------------------------------------------------- one frame's inputs and its launches
class Inputs:
    """frame f's inputs in buffers of their own, uploaded once.  `after`: the Inputs of the frame before it in the run when f is slot H there: frame, map
    and table are that frame's buffers, and the last frame is what it left in the block"""

    def __init__(self, N, f, after=None):
        from test_gpu_track import _device_frame
        self.f, c = f, f.c
        if after is None:
            self.F, self.fkeep = _device_frame(c["frame"])
            order = ("lm_obs_offsets", "lm_obs_kf", "lm_obs_octave", "lm_bad", "lm_nobs", "kf_bad", "kf_id")
            self.tkeep = [dev(c["T"][k]) for k in order]
            self.KT = N.KfTable(f.L, f.n_kf, *[b.ptr for b in self.tkeep])
            self.lms0 = np.zeros(f.L + f.new_cap, N.LM_DTYPE)
            self.lms0[:f.L] = c["lms"]
            self.lms0["skip"][f.L:] = 1
            self.d_lms = guarded(self.lms0)
            self.d_Tpred, self.d_last_kps, self.d_last_kp_lm = dev(np.ascontiguousarray(c["Tcw_pred"], np.float32)), dev(np.ascontiguousarray(c["last_kps"], N.KP_DTYPE)), dev(c["last_kp_lm"])
            self.last = (self.d_Tpred.ptr, self.d_last_kps.ptr, self.d_last_kp_lm.ptr)
        else:
            assert (after.f.n, after.f.L, after.f.new_cap) == (f.n_last, f.L, f.new_cap)
            self.F, self.KT, self.d_lms, self.lms0, self.last = after.F, after.KT, after.d_lms, after.lms0, None
        self.d_neigh, self.d_parent = dev(c["neigh"]), dev(c["parent"])
        tp = c["tp"]
        self.tp = N.TrackParams(tp.th_motion, tp.th_motion_wide, tp.n_min_matches, tp.th_local, tp.nnratio_motion, tp.nnratio_local, tp.th_high, tp.sigma_ref,
                                tp.n_max_local_keyframes, tp.n_neighbor_keyframes)
        if f.kf:
            K = f.kf["K"]
            self.kkeep = [dev(K["kf_off"]), dev(K["kp_lm"])]
            self.KF = N.KfFeatures(K["n_kf"], self.kkeep[0].ptr, None, None, None, self.kkeep[1].ptr, None)
            self.d_depth, self.d_ref, self.prm = dev(f.kf["depth"]), guarded(np.array([-1], np.int32)), N.KeyFrameParams(**f.kf["prm"])


def enqueue(tracker, N, blk, inp, s, st, last=None, track_only=False):
    """frame inp.f into the block on stream st, state set s.  `last`: (d_Tcw_pred, d_last_kps, d_last_kp_lm) when the inputs carry none (slot H in a run)"""
    f = inp.f
    ST = N.TrackState(*[blk.ptr("st%d.%s" % (s, k)) for k in STATE])
    names = lambda spec, prefix="": [blk.ptr(prefix + k) for k, _, _ in spec]
    out = N.TrackOut(*names(N.TRACK_OUT_HEAD), N.LocalMapOut(*names(N.LOCAL_MAP_OUT_SPEC, "local.")), *names(N.TRACK_OUT_TAIL))
    d_Tpred, d_last_kps, d_last_kp_lm = inp.last or last
    tracker.track_frame_device(inp.F, d_Tpred, d_last_kps, d_last_kp_lm, f.n_last, inp.KT, inp.d_lms.ptr, inp.d_neigh.ptr, 10, inp.d_parent.ptr, f.cap, inp.tp, ST, out,
                               blk.ptr("work"), st.ptr)
    if not f.kf or track_only:
        return
    kout = N.KeyFrameOut(*names(N.KEYFRAME_OUT_SPEC, "kf."), inp.d_lms.ptr, f.L + f.new_cap)
    d_Tcw = blk.ptr("pose_local", N.POSE_RESULT_DTYPE.fields["Tcw"][1])
    tracker.track_keyframe_device(inp.F, inp.d_depth.ptr, d_Tcw, inp.KT, inp.KF, blk.ptr("result"), inp.prm, ST, inp.d_ref.ptr, f.new_cap, kout, blk.ptr("kfwork"), st.ptr)
    tracker._ex.landmark_update_entries_device(f.new_cap, blk.ptr("kf.entries"), blk.ptr("kf.obs_offsets"), blk.ptr("kf.obs"), blk.ptr("kf.desc_offsets"), blk.ptr("kf.desc"),
                                               *[blk.ptr("eu.%d" % i) for i in range(8)], d_lms=inp.d_lms.ptr, d_lm_index=blk.ptr("kf.lm_index"),
                                               n_lms=f.L + f.new_cap, stream=st.ptr)


def results(N, blk, snap, f, s, kf=True):
    """the frame's outputs out of a snapshot of the block: field -> array at the frame's own sizes (copies)"""
    got = {k: view(snap, blk, k, dt, cnt).copy() for k, dt, cnt in track_fields(N, f)}
    for k, dt, cnt in state_fields(f, s):
        got[k.split(".")[1]] = view(snap, blk, k, dt, cnt).copy()
    if f.kf and kf:
        got.update({k: view(snap, blk, k, dt, cnt).copy() for k, dt, cnt in keyframe_fields(N, f.new_cap)})
    return got


def extents(tracker, N, blk, snap, f, s, kf=True):
    """-> {field: (bytes the frame may have written, bytes of them that are defined by the inputs alone)} from the counts the frame left in `snap`"""
    got = results(N, blk, snap, f, s, kf)
    ext = {}
    for k, dt, cnt in track_fields(N, f):
        ext[k] = (dt.itemsize * cnt,) * 2
    assert set(WHOLE) >= {k for k in ext if not k.startswith(("edges_", "outlier_"))}
    esz = N.POSE_EDGE_DTYPE.itemsize
    for stage in ("motion", "local"):
        ne = min(max(int(got["n_edges_" + stage][0]), 0), f.n)
        run = min(max(int(got["n_edges_motion"][1]), 0), f.n) if stage == "motion" else ne
        ext["edges_" + stage] = (ne * esz,) * 2
        ext["outlier_" + stage] = (run if run >= 3 else 0,) * 2             # not touched for a problem with fewer than 3 edges (include/hyslam_amd.h)
    for k, dt, cnt in state_fields(f, s):
        ext[k] = (dt.itemsize * cnt,) * 2
    ext["work"] = (tracker.track_work_bytes(f.n, f.n_last, f.L, f.cap), 0)
    if f.kf and kf:
        m = min(max(int(got["kf.result"][0]["n_new"]), 0), f.new_cap)
        for k, dt, cnt in keyframe_fields(N, f.new_cap):
            name = k[3:]
            ext[k] = (dt.itemsize * cnt,) * 2 if name in KF_WHOLE else (dt.itemsize * (cnt // max(f.new_cap, 1)) * m,) * 2
        ext["kf.result"] = (KF_RESULT_BYTES,) * 2                            # the ten named fields; no stage writes the record's _pad[6]
        for i, row in enumerate(EU):                                        # every row is written; the rows behind the last record come from records no call defined
            ext["eu.%d" % i] = (row * f.new_cap, row * m)
        ext["kfwork"] = (tracker.keyframe_work_bytes(f.n, f.n_kf, f.new_cap), 0)
    return ext


def defined_bytes(blk, snap, ext):
    return {k: snap[blk.off[k]:blk.off[k] + d].tobytes() for k, (w, d) in ext.items() if d}


def untouched(blk, before, after, ext, tag):
    """every byte the frame had no business writing is what it was before the frame, the guards included"""
    may = np.zeros(blk.total, bool)
    for k, (w, d) in ext.items():
        assert w <= blk.cap[k], (tag, k)
        may[blk.off[k]:blk.off[k] + w] = True
    bad = np.nonzero(~may & (before != after))[0]
    if len(bad):
        k = max((o, k) for k, o in blk.off.items() if o <= bad[0])[1]
        raise AssertionError("%s: byte %d of %s (capacity %d, the frame's extent %d) changed; %d bytes in all" % (tag, bad[0] - blk.off[k], k, blk.cap[k], ext.get(k, (0,))[0], len(bad)))
    assert (after[blk.pad] == blk.fill).all(), (tag, "guard bytes")


# ---------------------------------------------------------------- a case alone, computed once
_ALONE = {}


def alone(tracker, N, f, key):
    """frame f alone in fresh 0x55 buffers of exactly its sizes -> dict(pre: the tracking chain's results before the later stages, ext, bytes: the defined
    bytes of the full chain, lms, ref_slot).  Computed once per case and shared by every mode"""
    if key in _ALONE:
        return _ALONE[key]
    st, out = hipmem.Stream(), {}
    for track_only in (True, False):
        blk, inp = chain_block(tracker, N, [f], 0x55, 5), Inputs(N, f)
        before = blk.snapshot()
        enqueue(tracker, N, blk, inp, 0, st, track_only=track_only)
        st.synchronize()
        snap = blk.snapshot()
        ext = extents(tracker, N, blk, snap, f, 0, kf=not track_only)
        untouched(blk, before, snap, ext, ("alone", f.slot, track_only))
        if track_only:
            out["pre"] = results(N, blk, snap, f, 0, kf=False)
            compare_track(out["pre"], f.c, f.ref, "%s alone" % f.slot, N.LM_DTYPE)      # the state the tracking chain leaves, against the reference
            if not f.kf:
                break
    out.update(ext=ext, bytes=defined_bytes(blk, snap, ext), got=results(N, blk, snap, f, 0), lms=read(inp.d_lms, N.LM_DTYPE, f.L + f.new_cap))
    if f.kf:
        out["ref_slot"] = int(read(inp.d_ref, np.int32, 1)[0])
    _ALONE[key] = out
    return out


def rename(ext_or_bytes, s):
    """field names of state set s -> set 0 (what the case alone uses)"""
    return {k.replace("st%d." % s, "st0."): v for k, v in ext_or_bytes.items()}


# ---------------------------------------------------------------- the checks of one frame
_H = {}


def frame_h(g, g_got):
    """slot H from what G left on the DEVICE"""
    key = g_got["kp_lm"].tobytes() + g_got["pose_local"][0]["Tcw"].tobytes()
    if key not in _H:
        c, ref, ok = CR.derive_h(g, g_got["kp_lm"], g_got["pose_local"][0]["Tcw"])
        assert ok, "slot H, built from the device's outputs of G, does not qualify"
        _H[key] = CR.Frame("H", c, ref, CR.run()["H"].kf["insert"])
    return _H[key], key


def check_frame(tracker, N, blk, before, after, f, s, inp, tag):
    """(a) and (b) for one frame of a run; -> the defined bytes by field (state set named as set 0)"""
    key = f.h_key if f.slot == "H" else f.slot
    al = alone(tracker, N, f, key)
    ext = extents(tracker, N, blk, after, f, s)
    untouched(blk, before, after, ext, tag)
    got = results(N, blk, after, f, s)
    # (a) the tracking chain against the reference.  The later stages rewrite the state in place: the state the tracking chain left is the one the
    # case alone left (checked there against the reference), and the state after the later stages is held to ref_keyframe below
    pre = al["pre"]
    compare_track(dict(got, **{k: pre[k] for k in STATE}) if f.kf else got, f.c, f.ref, str(tag), N.LM_DTYPE)
    if f.kf:
        tres, pose = got["result"][0], got["pose_local"][0]
        case = CR.keyframe_case(f, (pre["kp_lm"], pre["kp_outl"], pre["n_matches"][0]), pose["Tcw"],
                                dict(status=int(tres["status"]), n_matches_map=int(tres["n_matches_map"]), n_inliers=int(tres["n_inliers"])))
        want = RKF.literal(case)
        kgot = {k[3:]: v for k, v in got.items() if k.startswith("kf.")}
        kgot.update(kp_lm=got["kp_lm"], kp_outl=got["kp_outl"], n_matches=int(got["n_matches"][0]), kp_lm_obs=got["kp_lm_obs"], ref_slot_mem=al["ref_slot"])
        compare_keyframe(kgot, want, f.new_cap, tag, behind=None)
        assert want["result"]["insert"] == int(f.kf["insert"] and want["result"]["ok"]), tag
        m = min(want["result"]["n_new"], f.new_cap)
        lms = inp_lms(N, inp, f)
        assert lms[:f.L].tobytes() == inp.lms0[:f.L].tobytes() and lms[f.L + m:].tobytes() == inp.lms0[f.L + m:].tobytes(), (tag, "landmark rows outside [L, L + n_new)")
        if m:
            ref = RL.update_entries(want["entries"], [want["obs"][k:k + 1] for k in range(m)], [want["desc"][k:k + 1] for k in range(m)])
            exp = inp.lms0[f.L:f.L + m].copy()
            exp["pos"], exp["assoc_kp"], exp["prev_angle"], exp["skip"] = want["new_pos"], -1, 0, 0
            exp["normal"], exp["min_dist"], exp["max_dist"], exp["size"], exp["desc"] = ref["normal"], ref["min_dist"], ref["max_dist"], ref["size"], want["desc"]
            for name in exp.dtype.names:
                assert RL.same(lms[f.L:f.L + m][name], exp[name]), (tag, name)
        assert lms.tobytes() == al["lms"].tobytes(), (tag, "the landmark array differs from the case alone")
        assert int(read(inp.d_ref, np.int32, 1)[0]) == al["ref_slot"] == want["result"]["ref_slot"], tag
    # (b) the case alone
    mine, theirs = rename(defined_bytes(blk, after, ext), s), al["bytes"]
    assert {k: d for k, (w, d) in rename(ext, s).items()} == {k: d for k, (w, d) in al["ext"].items()}, (tag, "the counts differ from the case alone")
    for k in theirs:
        assert mine[k] == theirs[k], (tag, k, "differs from the case alone in fresh buffers")
    assert set(mine) == set(theirs)
    return mine


def inp_lms(N, inp, f):
    return read(inp.d_lms, N.LM_DTYPE, f.L + f.new_cap)


# ---------------------------------------------------------------- the runs
def run_frames(tracker, order, fill, back_to_back=False, state_seed=5):
    """the frames of `order` through one block -> [defined bytes by field] per frame, every frame checked"""
    from hyslam_amd import _native as N
    frames = CR.ordered(order)
    blk = chain_block(tracker, N, frames, fill, state_seed)
    st = hipmem.Stream()
    inputs = []
    for i, f in enumerate(frames):
        inputs.append(Inputs(N, f, inputs[i - 1] if f.slot == "H" else None))
    snaps = [hipmem.DevBuf(blk.total, zero=False) for _ in frames] if back_to_back else None
    hipmem.sync()
    before, out, host = blk.snapshot(), [], []

    def last_of(i):                                               # slot H: the last frame is what frame i - 1 left in the block
        if frames[i].slot != "H":
            return None
        assert frames[i - 1].slot == "G"
        return blk.ptr("pose_local", N.POSE_RESULT_DTYPE.fields["Tcw"][1]), inputs[i - 1].F.kps, blk.ptr("st%d.kp_lm" % ((i - 1) % 2))

    def checked(i, before, after):
        f = frames[i]
        if f.slot == "H":                                         # the case and its reference from the device's G
            g_got = results(N, blk, before, frames[i - 1], (i - 1) % 2)
            f, key = frame_h(frames[i - 1], g_got)
            f.h_key = key
            inputs[i].f = f
        return check_frame(tracker, N, blk, before, after, f, i % 2, inputs[i], (order, hex(fill), "b2b" if back_to_back else "waited", i, f.slot))

    if back_to_back:
        for i, f in enumerate(frames):                            # no host call that waits from here ...
            enqueue(tracker, N, blk, inputs[i], i % 2, st, last_of(i))
            hipmem.copy_async(snaps[i].ptr, blk.buf.ptr, blk.total, st)
        st.synchronize()                                          # ... to here
        for i in range(len(frames)):
            after = snaps[i].to_numpy(np.uint8, blk.total)
            out.append(checked(i, before, after))
            before = after
    else:
        for i, f in enumerate(frames):
            enqueue(tracker, N, blk, inputs[i], i % 2, st, last_of(i))
            st.synchronize()
            after = blk.snapshot()
            out.append(checked(i, before, after))
            before = after
    slots = CR.ORDERS[order]
    assert out[slots.index("I")] == out[slots.index("A")], "slot I does not give slot A's bytes"
    return out


def test_waited_run_under_four_fills(tracker):
    """the table's order, a wait and a read after every frame; the block filled once with 0x55, 0x00, 0xFF, 0xA5; under the last three the library's own
    arena carries the byte too (hs_debug_poison), so the projection search's grid lists, d_winner and d_pangle start from it"""
    lib, t0, seen = tracker._ex._lib, time.time(), []
    before = lib.hs_debug_poison_violations()
    try:
        for k, fill in enumerate(FILLS):
            if fill != 0x55:
                assert lib.hs_debug_poison(fill) == 0
            seen.append(run_frames(tracker, "table", fill, state_seed=5 + k))
    finally:
        lib.hs_debug_poison(-1)
    assert lib.hs_debug_poison_violations() == before
    for k in range(1, len(FILLS)):
        assert seen[k] == seen[0], "the defined bytes under 0x%02X differ from those under 0x55" % FILLS[k]
    print("waited, four fills: %.2f s" % (time.time() - t0))


def test_back_to_back_on_a_fresh_handle(gpu, tracker):
    """ascending n first, then the rest: the handle's arena starts empty and the posed search's claim (grid lists by n, d_winner and d_pangle by n_last
    or cap) grows from B (33 views, 22 / 44 landmarks) to G (257, 130 / 320) to A (300, 200 / 400) to E (1025, 600 / 1225), so it regrows at least three
    times with earlier frames' kernels still queued on the caller's stream; a regrow drains that stream inside the library, the test
    itself makes no call that waits.  Every frame's snapshot is a device-to-device copy enqueued behind it; one wait at the end.  The same order waited
    gives the same bytes"""
    import hyslam_amd as HS
    t0 = time.time()
    fresh = HS.FrameTracker(HS.ORBExtractor(device=0))
    from hyslam_amd import _native as N
    for f in CR.ordered("ascending"):                             # the cases alone run on the module's handle first: nothing of them grows the fresh one
        if f.slot != "H":
            alone(tracker, N, f, f.slot)
    b2b = run_frames(fresh, "ascending", 0x55, back_to_back=True)
    waited = run_frames(tracker, "ascending", 0x55)
    assert b2b == waited
    print("back to back: %.2f s" % (time.time() - t0))


@pytest.mark.parametrize("order", ["reverse", "rotated"])
def test_other_orders(tracker, order):
    t0 = time.time()
    got = run_frames(tracker, order, 0x55)
    assert len(got) == len(CR.SLOTS)
    print("%s: %.2f s" % (order, time.time() - t0))


# ---------------------------------------------------------------- the reference-key-frame pair
def refkf_fields(tracker, f):
    n, L = f["n"], f["L"]
    return {"match_kf": f["kf_cap"] * 4, "op_view": n * 4, "op_lm": n * 4, "n_bow": 4, "st.kp_lm": n * 4, "st.kp_outl": n, "st.n_matches": 4,
            "work": tracker.track_refkf_work_bytes(n, f["kf_cap"], L)}


def refkf_inputs(N, f):
    from test_gpu_refkf import device_keyframes
    KF, keep = device_keyframes(f["K"])
    ins = dict(KF=KF, keep=keep, bad=dev(f["lm_bad"]), kps=dev(np.ascontiguousarray(f["kps"], N.KP_DTYPE)), desc=dev(f["desc"]), node=dev(f["node"]),
               slot=dev(np.array([f["kf_slot"]], np.int32)), s0=[dev(f["state0"][0]), dev(f["state0"][1]), dev(np.array([f["state0"][2]], np.int32))])
    ins["KT"] = N.KfTable(f["L"], 0, None, None, None, ins["bad"].ptr, None, None, None)
    return ins


def refkf_enqueue(tracker, blk, f, ins, st):
    """the frame's entry state into the shared state set (a device-to-device copy on the stream: no host wait), the search, the replay"""
    n = f["n"]
    for k, b, nbytes in zip(("st.kp_lm", "st.kp_outl", "st.n_matches"), ins["s0"], (n * 4, n, 4)):
        hipmem.copy_async(blk.ptr(k), b.ptr, nbytes, st)
    tracker.search_by_bow_kf_device(ins["KF"], ins["slot"].ptr, ins["KT"], ins["kps"].ptr, ins["desc"].ptr, ins["node"].ptr, None, n, f["th_low"], f["nnratio"],
                                    blk.ptr("match_kf"), f["kf_cap"], blk.ptr("op_view"), blk.ptr("op_lm"), blk.ptr("n_bow"), None, st.ptr)
    tracker.frame_associate_views_device(n, f["L"], blk.ptr("st.kp_lm"), blk.ptr("st.kp_outl"), blk.ptr("st.n_matches"), blk.ptr("op_view"), blk.ptr("op_lm"),
                                         blk.ptr("work"), st.ptr)


def refkf_check(tracker, blk, before, after, f, tag):
    need = refkf_fields(tracker, f)
    ext = {k: (b, 0 if k == "work" else b) for k, b in need.items()}
    untouched(blk, before, after, ext, tag)
    i32 = np.dtype(np.int32)
    got = [view(after, blk, "match_kf", i32, f["kf_cap"]), view(after, blk, "op_view", i32, f["n"]), view(after, blk, "op_lm", i32, f["n"]), int(view(after, blk, "n_bow", i32, 1)[0])]
    for g, w, what in zip(got, f["search"], ("match_kf", "op_view", "op_lm", "n_matches")):
        assert np.array_equal(g, w), (tag, what)
    state = view(after, blk, "st.kp_lm", i32, f["n"]), view(after, blk, "st.kp_outl", np.dtype(np.uint8), f["n"]), int(view(after, blk, "st.n_matches", i32, 1)[0])
    for g, w, what in zip(state, f["state"], ("kp_lm", "kp_outl", "n_matches")):
        assert np.array_equal(g, w), (tag, what)
    return defined_bytes(blk, after, ext)


def refkf_run(tracker, fill, back_to_back=False):
    from hyslam_amd import _native as N
    frames = CR.refkf_run()
    blk, st = Block(largest(refkf_fields(tracker, f) for f in frames), fill), hipmem.Stream()
    inputs = [refkf_inputs(N, f) for f in frames]
    snaps = [hipmem.DevBuf(blk.total, zero=False) for _ in frames] if back_to_back else None
    hipmem.sync()
    before, out = blk.snapshot(), []
    for i, f in enumerate(frames):
        refkf_enqueue(tracker, blk, f, inputs[i], st)
        if back_to_back:
            hipmem.copy_async(snaps[i].ptr, blk.buf.ptr, blk.total, st)
        else:
            st.synchronize()
            after = blk.snapshot()
            out.append(refkf_check(tracker, blk, before, after, f, ("refkf", hex(fill), i)))
            before = after
    if back_to_back:
        st.synchronize()
        for i, f in enumerate(frames):
            after = snaps[i].to_numpy(np.uint8, blk.total)
            out.append(refkf_check(tracker, blk, before, after, f, ("refkf b2b", i)))
            before = after
    return out


def test_refkf_run(tracker):
    """hs_search_by_bow_kf_device then hs_frame_associate_views_device at 130, 5, 1025, 64 and 257 views through one work area, one state set and one set
    of outputs: against ref_refkf on every frame, identical under the four fills (the reference IS the case alone here: every output is an integer array
    the reference gives in full), and back to back"""
    t0 = time.time()
    seen = [refkf_run(tracker, fill) for fill in FILLS]
    for k in range(1, len(FILLS)):
        assert seen[k] == seen[0], hex(FILLS[k])
    assert refkf_run(tracker, 0x55, back_to_back=True) == seen[0]
    print("refkf run: %.2f s" % (time.time() - t0))
