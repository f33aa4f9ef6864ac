"""The (real, decoy) pairs of tests/test_gpu_stream_order.py, built from the existing generators and references; tests/test_stream_order_cases.py holds
their properties on the CPU.

A Case is one entry-point call: device inputs as {key: (real, decoy)} of equal shape and dtype, the byte size of every output, the host arguments
(`args`, the same for both), and per output the bytes the call DEFINES with what the reference gives for the real and for the decoy inputs
(`expect`: {key: [(byte offset, real, decoy), ...]}).  Everything that lives on the device and that a kernel trusts (CSR offsets, indices, counts,
d_n, d_qm, d_n_edges) is valid in the decoy too: whatever order the work runs in, nothing reads out of range.  `primary`: the outputs that must tell the
two apart (all of `expect` unless named)."""
import functools

import numpy as np

import oracle
import ref_bow
import ref_kfgraph as RK
import ref_landmark
import ref_localmap as RL
import ref_place
import scenes
from hyslam_amd import _native as N
from hyslam_amd.synth import synth_stereo_pair
from kfgraph_cases import csr, random_candidates, random_table
from localmap_cases import random_keyframes

KB = N.KP_DTYPE.itemsize
TABLE_KEYS = ("lm_obs_offsets", "lm_obs_kf", "lm_obs_octave", "lm_bad", "lm_nobs", "kf_bad", "kf_id")


class Case:
    def __init__(self, kind, name, inputs, outputs, expect, args=None, primary=None, aux=None):
        self.kind, self.name, self.inputs, self.outputs, self.expect = kind, name, inputs, outputs, expect
        self.args, self.primary, self.aux = args or {}, tuple(primary or expect), aux or {}

    def __repr__(self):
        return "%s/%s" % (self.kind, self.name)


def pair(real, decoy):
    return np.ascontiguousarray(real), np.ascontiguousarray(decoy)


def whole(real, decoy):
    return [(0, np.ascontiguousarray(real), np.ascontiguousarray(decoy))]


def rows(real_rows, decoy_rows, row_bytes):
    """the defined prefix of every row of a [rows][cap] output: row i starts at i * row_bytes"""
    return [(i * row_bytes, np.ascontiguousarray(r), np.ascontiguousarray(d)) for i, (r, d) in enumerate(zip(real_rows, decoy_rows))]


def padded(a, n, dtype=None):
    out = np.zeros(n, dtype or a.dtype)
    out[:len(a)] = a
    return out


# ---------------------------------------------------------------- landmark representative descriptors
def _landmarks(seed, lengths):
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        base = rng.integers(0, 256, (3, 32), dtype=np.uint8)
        d = base[rng.integers(0, 3, n)].copy()
        flips = rng.integers(0, 256, (n, 4))
        for j in range(4):
            d[np.arange(n), flips[:, j] // 8] ^= (1 << (flips[:, j] % 8)).astype(np.uint8) * (rng.random(n) < 0.6).astype(np.uint8)
        out.append(d)
    return out


def _csr_desc(lms):
    off = np.zeros(len(lms) + 1, np.int64)
    np.cumsum([len(d) for d in lms], out=off[1:])
    return off, np.ascontiguousarray(np.concatenate(lms))


def landmark_case(path):
    """small: every landmark has N <= 64 observations (one wavefront each); large: some above 64 (the workgroup path).  The decoy has the same
    lengths in reverse order: other offsets, the same total"""
    rng = np.random.default_rng(5 if path == "small" else 6)
    lengths = rng.integers(0, 41, 300).tolist() if path == "small" else rng.integers(2, 30, 40).tolist()
    if path == "small":
        lengths[7], lengths[100] = 64, 63
    else:
        lengths[0], lengths[13], lengths[39] = 65, 300, 129
    real, decoy = _landmarks(11, lengths), _landmarks(12, lengths[::-1])
    (ro, rd), (do, dd) = _csr_desc(real), _csr_desc(decoy)
    (rb, rm), (db, dm) = ref_landmark.distinctive_descriptors_fast(real), ref_landmark.distinctive_descriptors_fast(decoy)
    L = len(lengths)
    return Case("landmark_best_descriptors", path, dict(offsets=pair(ro, do), desc=pair(rd, dd)), dict(best=4 * L, median=4 * L),
                dict(best=whole(rb.astype(np.int32), db.astype(np.int32)), median=whole(rm.astype(np.int32), dm.astype(np.int32))), args=dict(L=L))


# ---------------------------------------------------------------- key-frame graph
def mirrored_table(T, seed):
    """a second valid table of the same shapes: the landmarks in reverse order, every observing slot s as n_kf - 1 - s (rows stay ascending), other
    flags and ids"""
    rng = np.random.default_rng(seed)
    off, n_kf, L = T["lm_obs_offsets"], len(T["kf_id"]), len(T["lm_bad"])
    n = np.diff(off)[::-1]
    off2 = np.zeros(L + 1, np.int64)
    np.cumsum(n, out=off2[1:])
    kf2 = (n_kf - 1 - T["lm_obs_kf"])[::-1].astype(np.int32)        # reversing the whole array reverses the landmark order and every row
    oc2 = T["lm_obs_octave"][::-1].astype(np.int32)
    out = dict(lm_obs_offsets=off2, lm_obs_kf=np.ascontiguousarray(kf2), lm_obs_octave=np.ascontiguousarray(oc2),
               lm_bad=(rng.random(L) < 0.07).astype(np.uint8), lm_nobs=np.ascontiguousarray(T["lm_nobs"][::-1]),
               kf_bad=(rng.random(n_kf) < 0.07).astype(np.uint8), kf_id=(rng.permutation(n_kf).astype(np.int64) + 500))
    for k in TABLE_KEYS:
        assert out[k].shape == T[k].shape and out[k].dtype == T[k].dtype, k
    return out


def table_inputs(Tr, Td):
    return {"T." + k: pair(Tr[k], Td[k]) for k in TABLE_KEYS}


def _frame_queries(seed, L, sizes):
    rng = np.random.default_rng(seed)
    return csr([rng.integers(0, L, n) for n in sizes])


def kf_votes_case(which):
    """lds: n_kf <= HS_KF_LDS_SLOTS, the counters in LDS; global: one slot more, the weights rows ARE the counters (zeroed and counted with device
    atomics inside the call)"""
    n_kf = 64 if which == "lds" else N.HS_KF_LDS_SLOTS + 1
    L, sizes, th, cap = 400, [300, 0, 150, 40], 2, 12
    Tr = random_table(21, n_kf, L, max_obs=20, big=[(3, 64)], window=which != "lds")
    Td = mirrored_table(Tr, 22)
    (ro, rq), (do, dq) = _frame_queries(23, L, sizes), _frame_queries(24, L, sizes[::-1])
    ids_r = np.array([-1, -1, int(Tr["kf_id"][5]), -1], np.int64)
    ids_d = np.array([int(Td["kf_id"][9]), -1, -1, -1], np.int64)
    wr, wd = RK.votes_fast(Tr, ro, rq, ids_r, 0, th, cap), RK.votes_fast(Td, do, dq, ids_d, 0, th, cap)
    Q = len(sizes)
    inputs = dict(table_inputs(Tr, Td), q_offsets=pair(ro, do), q_lm=pair(rq, dq), q_self_id=pair(ids_r, ids_d))
    sizes_out = dict(weights=Q * n_kf, max_slot=Q, max_count=Q, ordered_slot=Q * cap, ordered_weight=Q * cap, n_ordered=Q)
    return Case("kf_votes", which, inputs, {k: 4 * n for k, n in sizes_out.items()}, {k: whole(wr[k], wd[k]) for k in RK.VOTE_KEYS},
                args=dict(L=L, n_kf=n_kf, Q=Q, count_bad_kf=0, th=th, cap=cap), primary=("weights", "ordered_slot", "ordered_weight", "max_count"))


def kf_redundancy_case():
    n_kf, L, sizes = 200, 600, [0, 64, 700, 1, 65]
    Tr = random_table(31, n_kf, L, max_obs=30, big=[(17, 150)])
    Td = mirrored_table(Tr, 32)
    cr, cd = random_candidates(33, Tr, sizes), random_candidates(34, Td, sizes[::-1])
    keys = ("cand_slot", "cand_th_depth", "cand_offsets", "item_lm", "item_octave", "item_depth")
    wr, wd = (RK.redundancy_fast(T, *[c[k] for k in keys], 0, 3, 0.9) for T, c in ((Tr, cr), (Td, cd)))
    C = len(sizes)
    inputs = dict(table_inputs(Tr, Td), **{k: pair(cr[k], cd[k]) for k in keys})
    return Case("kf_redundancy", "five", inputs, dict(n_mps=4 * C, n_redundant=4 * C, cull=C), {k: whole(wr[k], wd[k]) for k in RK.RED_KEYS},
                args=dict(L=L, n_kf=n_kf, C=C, is_mono=0, th_obs=3, frac=0.9), primary=("n_mps", "n_redundant"))


# ---------------------------------------------------------------- local map
def local_keyframes_case():
    n_kf, neigh_cap = 129, 10
    r, d = random_keyframes(41, n_kf, neigh_cap), random_keyframes(42, n_kf, neigh_cap)
    n_max, n_neighbor = 80, 6
    keys = ("weights", "kf_bad", "neigh", "parent")
    (lr, nr), (ld, nd) = (RL.local_keyframes_fast(*[c[k] for k in keys], n_max, n_neighbor) for c in (r, d))
    return Case("local_keyframes", "129", {k: pair(r[k], d[k]) for k in keys}, dict(local=n_kf, n_local=4),
                dict(local=whole(lr.astype(np.uint8), ld.astype(np.uint8)), n_local=whole(np.array([nr], np.int32), np.array([nd], np.int32))),
                args=dict(n_kf=n_kf, neigh_cap=neigh_cap, n_max=n_max, n_neighbor=n_neighbor))


def _points_inputs(seed, T, n_assoc, p_local):
    rng = np.random.default_rng(seed)
    L, n_kf = len(T["lm_bad"]), len(T["kf_id"])
    local = (rng.random(n_kf) < p_local).astype(np.uint8)
    flm = rng.integers(0, L, n_assoc).astype(np.int32)
    flm[rng.random(n_assoc) < 0.2] = -1
    flm[-1] = flm[0]
    return local, flm


def local_points_case():
    """L = 3 compaction blocks and one landmark: more than one workgroup, a partial last block"""
    n_kf, L, n_assoc = 100, 3 * N.HS_LOCAL_POINTS_BLOCK + 1, 200
    Tr = random_table(51, n_kf, L, max_obs=12, big=[(3, 90)], p_bad_lm=0.1)
    Td = mirrored_table(Tr, 52)
    (lr, fr), (ld, fd) = _points_inputs(53, Tr, n_assoc, 0.15), _points_inputs(54, Td, n_assoc, 0.2)
    cap = L
    wr, wd = RL.local_points_fast(Tr, lr, fr, cap), RL.local_points_fast(Td, ld, fd, cap)
    i32 = lambda v: np.array([v], np.int32)
    # sel is defined up to min(n_sel, cap); the -1 padding behind it is written too (ref_localmap.pack_points)
    return Case("local_points", "3blocks+1", dict(table_inputs(Tr, Td), local=pair(lr, ld), frame_lm=pair(fr, fd)),
                dict(frame_remove=n_assoc, sel=4 * cap, n_sel=4),
                dict(frame_remove=whole(wr["frame_remove"], wd["frame_remove"]), sel=whole(wr["sel"], wd["sel"]), n_sel=whole(i32(wr["n_sel"]), i32(wd["n_sel"]))),
                args=dict(L=L, n_kf=n_kf, n_assoc=n_assoc, cap=cap), primary=("sel", "n_sel"))


def landmark_gather_case():
    L, cap = 401, 64
    out = []
    for seed, n_sel in ((61, 37), (62, 50)):
        rng = np.random.default_rng(seed)
        lms = np.frombuffer(rng.integers(0, 256, L * N.LM_DTYPE.itemsize, dtype=np.uint8).tobytes(), N.LM_DTYPE).copy()
        sel = np.full(cap, -1, np.int32)
        sel[:n_sel] = np.sort(rng.choice(L, n_sel, replace=False))
        out.append((lms, sel, np.array([n_sel], np.int32), RL.gather(lms, sel, n_sel, cap)))
    r, d = out
    return Case("landmark_gather", "37of64", dict(lms=pair(r[0], d[0]), sel=pair(r[1], d[1]), n_sel=pair(r[2], d[2])), dict(out=cap * N.LM_DTYPE.itemsize),
                dict(out=whole(r[3], d[3])), args=dict(L=L, cap=cap))


# ---------------------------------------------------------------- the extractor and the stereo front end (the oracle, as tests/test_gpu_parity.py)
W, H, NF = 640, 480, 1000
STEREO = dict(fx=500.0, mbf=60.0, n_rows=H, th_high=100.0, th_low=50.0, size_ref=31.0)


@functools.lru_cache(maxsize=None)
def stereo_pair_ref(seed):
    """(left, right, kL, dL, kR, dR, uRight, depth) of one 640 x 480 pair, the reference's answers from the oracle: computed once per seed"""
    L, R = synth_stereo_pair(seed, W, H)
    return (L, R) + tuple(np.ascontiguousarray(a) for a in oracle.stereo_frontend(oracle.default_params(NF), oracle.stereo_params(**STEREO), L, R))


def _feature_rows(feats, cap):
    """[(kps, desc)] per frame -> the expect segments of kps [B][cap], desc [B][cap][32], n [B]"""
    return [k for k, _ in feats], [d for _, d in feats], np.array([len(k) for k, _ in feats], np.int32)


def extract_case(cap, seeds=(7, 8)):
    """2 frames of 640 x 480 (a stereo pair's two views); the decoy is another pair.  cap: hs_orb_max_keypoints() of the handle (the row stride of the
    outputs); the reference does not depend on it"""
    r, d = stereo_pair_ref(seeds[0]), stereo_pair_ref(seeds[1])
    fr, fd = [(r[2], r[3]), (r[4], r[5])], [(d[2], d[3]), (d[4], d[5])]
    (kr, dr, nr), (kd, dd, nd) = _feature_rows(fr, cap), _feature_rows(fd, cap)
    assert max(nr.max(), nd.max()) <= cap
    return Case("extract_batch", "2x640x480 s%d" % seeds[0], dict(imgs=pair(np.stack(r[:2]), np.stack(d[:2]))), dict(kps=2 * cap * KB, desc=2 * cap * 32, n=8),
                dict(kps=rows(kr, kd, cap * KB), desc=rows(dr, dd, cap * 32), n=whole(nr, nd)), args=dict(batch=2, w=W, h=H, cap=cap))


def stereo_frontend_case(cap, seeds=((7, 9), (8, 10))):
    """2 pairs of 640 x 480 through extraction and the matcher in one call"""
    r, d = [stereo_pair_ref(s) for s in seeds[0]], [stereo_pair_ref(s) for s in seeds[1]]
    inputs = dict(left=pair(np.stack([x[0] for x in r]), np.stack([x[0] for x in d])), right=pair(np.stack([x[1] for x in r]), np.stack([x[1] for x in d])))
    P = len(r)
    outputs = dict(kpsL=P * cap * KB, descL=P * cap * 32, nL=4 * P, kpsR=P * cap * KB, descR=P * cap * 32, nR=4 * P, uRight=P * cap * 4, depth=P * cap * 4)
    col = lambda xs, i: [x[i] for x in xs]
    n = lambda xs, i: np.array([len(x[i]) for x in xs], np.int32)
    expect = dict(kpsL=rows(col(r, 2), col(d, 2), cap * KB), descL=rows(col(r, 3), col(d, 3), cap * 32), nL=whole(n(r, 2), n(d, 2)),
                  kpsR=rows(col(r, 4), col(d, 4), cap * KB), descR=rows(col(r, 5), col(d, 5), cap * 32), nR=whole(n(r, 4), n(d, 4)),
                  uRight=rows(col(r, 6), col(d, 6), cap * 4), depth=rows(col(r, 7), col(d, 7), cap * 4))
    return Case("stereo_frontend", "2 pairs", inputs, outputs, expect, args=dict(pairs=P, w=W, h=H, cap=cap, sp=STEREO))


def stereo_match_case():
    """3 pairs of keypoint lists with different counts laid out with stride cap, as the extractor leaves them"""
    r, d = [stereo_pair_ref(s) for s in (7, 9, 8)], [stereo_pair_ref(s) for s in (10, 8, 7)]
    cap = max(len(x[i]) for x in r + d for i in (2, 4)) + 3
    P = len(r)

    def layout(xs):
        kL, kR = np.zeros((P, cap), N.KP_DTYPE), np.zeros((P, cap), N.KP_DTYPE)
        dL, dR = np.zeros((P, cap, 32), np.uint8), np.zeros((P, cap, 32), np.uint8)
        for j, x in enumerate(xs):
            kL[j, :len(x[2])], dL[j, :len(x[2])], kR[j, :len(x[4])], dR[j, :len(x[4])] = x[2], x[3], x[4], x[5]
        return dict(kpsL=kL, descL=dL, nL=np.array([len(x[2]) for x in xs], np.int32), kpsR=kR, descR=dR, nR=np.array([len(x[4]) for x in xs], np.int32))
    a, b = layout(r), layout(d)
    col = lambda xs, i: [x[i] for x in xs]
    return Case("stereo_match", "3 pairs", {k: pair(a[k], b[k]) for k in a}, dict(uRight=P * cap * 4, depth=P * cap * 4),
                dict(uRight=rows(col(r, 6), col(d, 6), cap * 4), depth=rows(col(r, 7), col(d, 7), cap * 4)), args=dict(pairs=P, cap=cap, sp=STEREO))


def preprocess_case():
    """2 BGR frames of 333 x 201 with 5 bytes of row padding (the byte-load path), scale 0.75 (bilinear), grey rows padded by 3"""
    w, h, cn, padb, batch, scale, rgb = 333, 201, 3, 5, 2, 0.75, False
    ow, oh = oracle.preprocess_size(w, h, scale)
    row, gpitch = w * cn + padb, ow + 3
    srcs, greys = [], []
    for seed in (71, 72):
        rng = np.random.default_rng(seed)
        frames = [rng.integers(0, 256, (h, w, cn), dtype=np.uint8) for _ in range(batch)]
        src = np.zeros((batch, h, row), np.uint8)
        for i, f in enumerate(frames):
            src[i, :, :w * cn] = f.reshape(h, w * cn)
        srcs.append(src)
        greys.append(np.concatenate([oracle.preprocess(f, rgb, scale) for f in frames]))         # [batch * oh][ow]
    return Case("preprocess", "333x201x3", dict(src=pair(*srcs)), dict(grey=batch * oh * gpitch), dict(grey=rows(list(greys[0]), list(greys[1]), gpitch)),
                args=dict(w=w, h=h, row=row, batch=batch, cn=cn, rgb=rgb, scale=scale, gpitch=gpitch, oh=oh))


# ---------------------------------------------------------------- projection search, pose edges and pose optimisation
PROJ = (5.0, 100.0, 0.8, 0.5, 1.5, 1, 1, 0)                       # SearchByProjection(Frame, MapPoints, th = 5): the local-map criteria


@functools.lru_cache(maxsize=None)
def projection_scene():
    return scenes.projection_scene(61, W, H, nfeat=300, copies=3)


def _reversed_frame(fa):
    """the same pose and camera (host arguments of the call), the keypoints in reverse order: a valid frame whose every index differs"""
    return dict(fa, kps=np.ascontiguousarray(fa["kps"][::-1]), desc=np.ascontiguousarray(fa["desc"][::-1]), uR=np.ascontiguousarray(fa["uR"][::-1]),
                kp_lm_obs=np.ascontiguousarray(fa["kp_lm_obs"][::-1]))


def _frame_inputs(fr, fd):
    return {"F.kps": pair(np.ascontiguousarray(fr["kps"], N.KP_DTYPE), np.ascontiguousarray(fd["kps"], N.KP_DTYPE)), "F.desc": pair(fr["desc"], fd["desc"]),
            "F.uR": pair(np.asarray(fr["uR"], np.float32), np.asarray(fd["uR"], np.float32)),
            "F.kp_lm_obs": pair(np.asarray(fr["kp_lm_obs"], np.int32), np.asarray(fd["kp_lm_obs"], np.int32))}


def _decoy_landmarks(lms, n):
    """reversed, the held keypoints renumbered for the reversed frame"""
    out = np.ascontiguousarray(lms[::-1])
    held = out["assoc_kp"] >= 0
    out["assoc_kp"][held] = n - 1 - out["assoc_kp"][held]
    return out


def projection_case(posed):
    """hs_search_by_projection_device; posed: the pose comes from device memory (hs_pose_view), the decoy's from another pose"""
    sc = projection_scene()
    fr = sc["frame_args"]
    fd = _reversed_frame(fr)
    lr = np.ascontiguousarray(sc["lms"], N.LM_DTYPE)
    ld = _decoy_landmarks(lr, len(fr["kps"]))
    L = len(lr)
    pp = oracle.ProjParams(*PROJ)
    inputs = dict(_frame_inputs(fr, fd), lms=pair(lr, ld))
    fd_pose = fd
    if posed:
        Rd = (scenes.small_rotation(0.003, -0.002, 0.004) @ np.asarray(fr["Rcw"], np.float32).reshape(3, 3)).astype(np.float32)
        fd_pose = dict(fd, Rcw=Rd, tcw=(np.asarray(fr["tcw"], np.float32) + np.float32(0.01)).astype(np.float32))
        views = []
        for f in (fr, fd_pose):
            Fh, _ = oracle.make_frame_view(N.FrameView, **f)
            pv = np.zeros(1, N.POSE_VIEW_DTYPE)
            pv["Rcw"][0], pv["tcw"][0], pv["Ow"][0] = list(Fh.Rcw), list(Fh.tcw), list(Fh.Ow)
            views.append(pv)
        inputs["pose"] = pair(*views)
    res = []
    for f, lms in ((fr, lr), (fd_pose, ld)):
        Fo, _ = oracle.make_frame_view(oracle.FrameView, **f)
        res.append(oracle.search_by_projection(Fo, lms, pp))
    (ri, rdist, rn), (di, ddist, dn) = res
    assert rn > 50 and dn > 50
    i32 = lambda v: np.array([v], np.int32)
    # match_dist is defined where match_idx >= 0 only (a dropped entry keeps its distance: the device form documents it): compared there by `aux`
    return Case("projection_posed" if posed else "projection", "local map", inputs, dict(match_idx=4 * L, match_dist=4 * L, n_matches=4),
                dict(match_idx=whole(ri, di), n_matches=whole(i32(rn), i32(dn))), args=dict(L=L, frame=fr, proj=PROJ),
                primary=("match_idx", "n_matches") if posed else ("match_idx",),       # not posed: the decoy is a renumbering, the count is the same
                aux=dict(match_dist=(np.asarray(rdist, np.float32), np.asarray(ddist, np.float32)), match_idx=(ri, di)))


def _kp_lm(fa, lms):
    """for every keypoint the landmark that projects nearest to it, within 2 px (tests/test_gpu_poseopt.py frame_scene), with entries outside [0, L)"""
    Rcw, tcw = np.asarray(fa["Rcw"], np.float64).reshape(3, 3), np.asarray(fa["tcw"], np.float64)
    Pc = lms["pos"].astype(np.float64) @ Rcw.T + tcw
    z = np.where(Pc[:, 2] > 0.1, Pc[:, 2], np.inf)
    uv = np.stack([fa["fx"] * Pc[:, 0] / z + fa["cx"], fa["fy"] * Pc[:, 1] / z + fa["cy"]], 1)
    kps = fa["kps"]
    d2 = (kps["x"][:, None] - uv[None, :, 0]) ** 2 + (kps["y"][:, None] - uv[None, :, 1]) ** 2
    near = d2.argmin(1)
    kp_lm = np.where(d2[np.arange(len(kps)), near] < 4.0, near, -1).astype(np.int32)
    held = np.nonzero(kp_lm >= 0)[0]
    kp_lm[held[3]], kp_lm[held[10]], kp_lm[held[20]] = len(lms), len(lms) + 7, -7
    return kp_lm


def pose_edges_case():
    import ref_poseopt
    sc = projection_scene()
    fr = sc["frame_args"]
    fd = _reversed_frame(fr)
    lr = np.ascontiguousarray(sc["lms"], N.LM_DTYPE)
    ld = _decoy_landmarks(lr, len(fr["kps"]))
    kr, kd = _kp_lm(fr, lr), _kp_lm(fd, ld)
    kd[np.nonzero(kd >= 0)[0][30:41]] = -1                        # the decoy holds eleven landmarks fewer: another count
    (er, cr), (ed, cd) = (ref_poseopt.gather_edges(f["kps"], f["uR"], k, l["pos"], size_ref=31.0, sigma_ref=1.0) for f, k, l in ((fr, kr, lr), (fd, kd, ld)))
    assert cr == len(er) > 100 and cd == len(ed) > 100
    cap = max(cr, cd) + 20
    esz = N.POSE_EDGE_DTYPE.itemsize
    i32 = lambda v: np.array([v], np.int32)
    inputs = {"F.kps": _frame_inputs(fr, fd)["F.kps"], "F.uR": _frame_inputs(fr, fd)["F.uR"], "lms": pair(lr, ld), "kp_lm": pair(kr, kd)}
    return Case("pose_edges", "640x480", inputs, dict(edges=cap * esz, n_edges=4),
                dict(edges=whole(np.ascontiguousarray(er, N.POSE_EDGE_DTYPE), np.ascontiguousarray(ed, N.POSE_EDGE_DTYPE)), n_edges=whole(i32(cr), i32(cd))),
                args=dict(L=len(lr), frame=fr, cap=cap, sigma_ref=1.0))


def pose_optimize_case():
    """Q = 1 with the edge count read from the device: 257 edges (two workgroup rounds and one edge) against a decoy of 120"""
    import poseopt_cases as P
    g = P.load_golden()
    names, cap = ("n257", "mixed_out30"), 300
    prob, edges, n, ref = [], [], [], []
    for name in names:
        T, cam, e = g[name + ".T"], g[name + ".cam"], g[name + ".edges"]
        p = np.zeros(1, N.POSE_PROBLEM_DTYPE)
        p["Tcw"][0] = np.asarray(T, np.float32).reshape(16)
        for k, v in zip(("fx", "fy", "cx", "cy", "bf"), cam):
            p[k][0] = v
        prob.append(p); edges.append(padded(np.ascontiguousarray(e, N.POSE_EDGE_DTYPE), cap)); n.append(np.array([len(e)], np.int32))
        ref.append({k: g[name + "." + k] for k in P.REF_KEYS})
    # the result record is compared as tests/test_gpu_poseopt.py compares it (Tcw_d within tau): by `aux`; the flags exactly
    return Case("pose_optimize", "n257", dict(problems=pair(*prob), edges=pair(*edges), n_edges=pair(*n)), dict(outlier=cap, results=N.POSE_RESULT_DTYPE.itemsize),
                dict(outlier=whole(ref[0]["outlier"].astype(np.uint8), ref[1]["outlier"].astype(np.uint8))), args=dict(cap=cap),
                aux=dict(ref=ref, tau=float(g["tau"])))


# ---------------------------------------------------------------- brute-force 2-NN, frame records, the vocabulary
def knn2_case():
    out = []
    for seed in (81, 82):
        rng = np.random.default_rng(seed)
        q, t = rng.integers(0, 256, (321, 32), dtype=np.uint8), rng.integers(0, 256, (517, 32), dtype=np.uint8)
        t[5:200] = scenes.flip_bits(rng, q[100:295], rng.integers(0, 20, 195))
        t[300] = t[5]
        out.append((q, t, ref_bow.hamming_knn2(q, t)))
    (qr, tr, rr), (qd, td, rd) = out
    return Case("hamming_knn2", "321x517", dict(q=pair(qr, qd), t=pair(tr, td)), dict(best_idx=4 * 321, best_dist=4 * 321, second_dist=4 * 321),
                {k: whole(rr[i], rd[i]) for i, k in enumerate(("best_idx", "best_dist", "second_dist"))}, args=dict(nq=321, nt=517))


@functools.lru_cache(maxsize=None)
def vocab_tree():
    """the "ragged" edge tree of scenes.vocab_edge_trees (levels of 1, 2, 5 and 17 children, leaves above the last level) with its descriptors"""
    return next(e for e in scenes.vocab_edge_trees(0) if e["name"] == "ragged")


LEVELSUP = 1


def _record_set(seed, index):
    return list(scenes.record_edge_sets(seed, pool=vocab_tree()["tree"]["desc"]))[index]


def records_knn2_case(index=5):
    """one process, several records in the all-gather layout (scenes.record_edge_sets): the counts are read from the record headers on the device.
    The `rank` row and the entries behind the query count are not written: they are no part of `expect`"""
    r, d = _record_set(9, index), _record_set(10, index)
    assert (r["world"], r["rank"], r["cap"], r["stride"]) == (d["world"], d["rank"], d["cap"], d["stride"])
    world, rank, cap = r["world"], r["rank"], r["cap"]
    expect = {k: [] for k in ("best_idx", "best_dist", "second_dist")}
    for peer in range(world):
        if peer == rank:
            continue
        a, b = (ref_bow.hamming_knn2(s["frames"][rank][1], s["frames"][peer][1]) for s in (r, d))
        for i, k in enumerate(expect):
            expect[k].append((peer * cap * 4, a[i], b[i]))
    return Case("records_knn2", "set %d" % index, dict(records=pair(r["buf"], d["buf"])), {k: world * cap * 4 for k in expect}, expect,
                args=dict(world=world, rank=rank, cap=cap, stride=r["stride"]))


def records_bow_match_case(index):
    """5: world 5, cap 301 (the call that grows the vocabulary's scratch); 4: world 5, cap 64 (the smaller call behind it)"""
    r, d = _record_set(9, index), _record_set(10, index)
    world, rank, cap = r["world"], r["rank"], r["cap"]
    thr, ratio, rot = 50.0, 0.9, 1
    t = vocab_tree()["tree"]
    (mr, nr), (md, nd) = (ref_bow.records_bow_match(t, LEVELSUP, s["frames"], rank, cap, thr, ratio, rot) for s in (r, d))
    return Case("records_bow_match", "set %d" % index, dict(records=pair(r["buf"], d["buf"])), dict(match12=world * cap * 4, n_matches=world * 4),
                dict(match12=whole(mr, md), n_matches=whole(nr, nd)), args=dict(world=world, rank=rank, cap=cap, stride=r["stride"], thr=thr, ratio=ratio, rot=rot))


def _tree_descs(seed, n):
    e = vocab_tree()
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(scenes.flip_bits(rng, e["desc"][rng.integers(0, len(e["desc"]), n)], rng.integers(0, 12, n)))


def bow_transform_case(n_max, counts):
    """the count is read from the device and clamped to n_max: counts = (real, decoy)"""
    t = vocab_tree()["tree"]
    dr, dd = _tree_descs(91 + n_max, n_max), _tree_descs(92 + n_max, n_max)
    rr, rd = ref_bow.bow_transform(t, dr[:counts[0]], LEVELSUP), ref_bow.bow_transform(t, dd[:counts[1]], LEVELSUP)
    i32 = lambda v: np.array([v], np.int32)
    return Case("bow_transform", "n_max %d" % n_max, dict(desc=pair(dr, dd), n=pair(i32(counts[0]), i32(counts[1]))), dict(word=4 * n_max, weight=4 * n_max, node=4 * n_max),
                {k: whole(rr[i], rd[i]) for i, k in enumerate(("word", "weight", "node"))}, args=dict(n_max=n_max), aux=dict(ref=(rr, rd)))


def bow_vector_case(n_max, counts):
    """n_max above 4096: the kernel asks for more than the default LDS"""
    n_words = 4 * n_max
    ins, refs = [], []
    for seed, n in zip((95 + n_max, 96 + n_max), counts):
        rng = np.random.default_rng(seed)
        word = rng.integers(0, n_words, n_max).astype(np.int32)
        weight = (rng.random(n_max) * 10 ** rng.uniform(-2, 2, n_max)).astype(np.float32)
        weight[rng.random(n_max) < 0.1] = 0.0
        w, v = ref_place.bow_vector(word[:n], weight[:n])
        ins.append((word, weight, np.array([n], np.int32)))
        refs.append((np.array(w, np.int32), np.array(v, np.float64), np.array([len(w)], np.int32)))
    (a, b), (ra, rb) = ins, refs
    return Case("bow_vector", "n_max %d" % n_max, dict(word=pair(a[0], b[0]), weight=pair(a[1], b[1]), n=pair(a[2], b[2])),
                dict(out_word=4 * n_max, out_value=8 * n_max, m=4), dict(out_word=whole(ra[0], rb[0]), out_value=whole(ra[1], rb[1]), m=whole(ra[2], rb[2])),
                args=dict(n_max=n_max))


# ---------------------------------------------------------------- the fused local-map call
def _local_map_inputs(seed, fa, lms, T):
    """neighbour rows (each slot's best covisible key frames), parents, and a frame that holds 60 entries: null, bad and good ones"""
    from kfgraph_cases import key_frame_queries
    rng = np.random.default_rng(seed)
    n_kf, L = len(T["kf_id"]), len(lms)
    off, q_lm, ids = key_frame_queries(T)
    neigh = np.ascontiguousarray(RK.votes_fast(T, off, q_lm, ids, 0, 3, 10)["ordered_slot"], np.int32)
    parent = np.full(n_kf, -1, np.int32)
    parent[rng.choice(n_kf, 4, replace=False)] = rng.integers(0, n_kf, 4)
    flm = rng.choice(L, 60, replace=False).astype(np.int32)
    flm[::9] = -1
    return neigh, parent, flm


def _local_map_ref(fa, lms, T, neigh, parent, flm, cap):
    held = flm[flm >= 0]
    w = RK.votes_fast(T, np.array([0, len(held)], np.int64), held, None, 1, 1, 0)
    out = dict(weights=w["weights"][0], max_slot=w["max_slot"][:1], max_count=w["max_count"][:1])
    local, n_local = RL.local_keyframes_fast(out["weights"], T["kf_bad"], neigh, parent, 80, 10)
    pts = RL.local_points_fast(T, local, flm, cap)
    gathered = RL.gather(lms, pts["sel"], pts["n_sel"], cap)
    Fo, _ = oracle.make_frame_view(oracle.FrameView, **fa)
    mi, md, mn = oracle.search_by_projection(Fo, gathered, oracle.ProjParams(*PROJ))
    i32 = lambda v: np.array([v], np.int32)
    out.update(local=local.astype(np.uint8), n_local=i32(n_local), frame_remove=pts["frame_remove"], sel=pts["sel"], n_sel=i32(pts["n_sel"]), lms=gathered,
               match_idx=mi, match_dist=np.asarray(md, np.float32), n_matches=i32(mn))
    return out


LOCAL_MAP_OUT = ("weights", "max_slot", "max_count", "local", "n_local", "frame_remove", "sel", "n_sel", "lms", "match_idx", "match_dist", "n_matches")


def local_map_search_case():
    """vote, key-frame expansion, landmark selection, gather and projection search in one call, on the 640 x 480 scene of the projection cases with a
    map of 65 key frames"""
    sc = projection_scene()
    fr = sc["frame_args"]
    fd = _reversed_frame(fr)
    lr = np.ascontiguousarray(sc["lms"], N.LM_DTYPE)
    ld = _decoy_landmarks(lr, len(fr["kps"]))
    L, n_kf = len(lr), 65
    Tr = random_table(71, n_kf, L, max_obs=6, window=True, p_bad_lm=0.08, p_bad_kf=0.1)
    Td = mirrored_table(Tr, 72)
    (ngr, par, flr), (ngd, pad, fld) = _local_map_inputs(73, fr, lr, Tr), _local_map_inputs(74, fd, ld, Td)
    cap = L
    rr, rd = _local_map_ref(fr, lr, Tr, ngr, par, flr, cap), _local_map_ref(fd, ld, Td, ngd, pad, fld, cap)
    assert int(rr["n_sel"][0]) > 50 and int(rr["n_matches"][0]) > 10 and int(rd["n_matches"][0]) > 10
    inputs = dict(table_inputs(Tr, Td), **_frame_inputs(fr, fd), frame_lm=pair(flr, fld), neigh=pair(ngr, ngd), parent=pair(par, pad), map_lms=pair(lr, ld))
    outputs = {k: np.ascontiguousarray(rr[k]).nbytes for k in LOCAL_MAP_OUT}
    exact = [k for k in LOCAL_MAP_OUT if k != "match_dist"]       # match_dist where match_idx >= 0, by `aux`
    return Case("local_map_search", "640x480", inputs, outputs, {k: whole(rr[k], rd[k]) for k in exact},
                args=dict(L=L, n_kf=n_kf, n_assoc=len(flr), neigh_cap=10, cap=cap, frame=fr, proj=PROJ),
                primary=("weights", "local", "sel", "lms", "match_idx"), aux=dict(match_dist=(rr["match_dist"], rd["match_dist"]), match_idx=(rr["match_idx"], rd["match_idx"])))


# ---------------------------------------------------------------- place recognition
def _padded_vec(w, v, m_max):
    assert len(w) <= m_max
    return padded(np.asarray(w, np.int32), m_max), padded(np.asarray(v, np.float64), m_max), np.array([len(w)], np.int32)


def _per_slot(slot_of, n_slots, det):
    """the restatement's dicts by key -> the library's per-slot arrays (tests/test_gpu_place.py per_slot)"""
    words, score, acc, best = np.full(n_slots, -1, np.int32), np.zeros(n_slots, np.float32), np.zeros(n_slots, np.float32), np.full(n_slots, -1, np.int32)
    for k, s in slot_of.items():
        if k in det["words"]:
            words[s], score[s] = det["words"][k], det["score"][k]
        if k in det["best"]:
            acc[s], best[s] = det["acc"][k], slot_of[det["best"][k]]
    return dict(words=words, score=score, acc=acc, best=best)


def _query_expect(slot_of, n_slots, keys, det):
    out = _per_slot(slot_of, n_slots, det)
    out["cand"] = np.array([slot_of[k] for k in keys], np.int32)
    out["n_cand"] = np.array([len(keys)], np.int32)
    return out


QUERY_OUT = ("cand", "n_cand", "words", "score", "acc", "best")


def _query_case(name, loop, slot_of, n_slots, refs, queries, neigh_tables, excludes, min_score, qm_max):
    """refs: the two restatement databases; queries: the two (words, values); -> the Case of one hs_place_query_*_device call"""
    exp = []
    for ref, (w, v), neigh_of, excl in zip(refs, queries, neigh_tables, excludes):
        key_of = {s: k for k, s in slot_of.items()}
        nb = {k: [key_of[int(x)] for x in neigh_of[slot_of[k]] if x >= 0] for k in slot_of}      # in the row's order
        if loop:
            connected = [k for k, s in slot_of.items() if excl[s]]
            keys, det = ref.detect_loop(w, v, connected, min_score, nb)
        else:
            keys, det = ref.detect_reloc(w, v, nb)
        exp.append(_query_expect(slot_of, n_slots, keys, det))
    a, b = (_padded_vec(w, v, qm_max) for w, v in queries)
    inputs = dict(qword=pair(a[0], b[0]), qvalue=pair(a[1], b[1]), qm=pair(a[2], b[2]), neigh=pair(*neigh_tables))
    if loop:
        inputs["exclude"] = pair(*excludes)
    outputs = dict(cand=4 * n_slots, n_cand=4, words=4 * n_slots, score=4 * n_slots, acc=4 * n_slots, best=4 * n_slots)
    return Case("place_query_loop" if loop else "place_query_reloc", name, inputs, outputs, {k: whole(exp[0][k], exp[1][k]) for k in QUERY_OUT},
                args=dict(qm_max=qm_max, slots=n_slots, min_score=min_score), primary=("words", "score"))


def _perturbed(rng, w0, n_words):
    keep = w0[rng.random(len(w0)) < 0.9]
    w = np.unique(np.concatenate([keep, rng.choice(n_words, size=max(1, len(w0) // 8), replace=False)])).astype(np.int32)
    v = rng.random(len(w)) + 0.05
    return w, v / v.sum()


def place_scene():
    """a database of 30 key frames added through the host form (before anything is held back), then on the caller's stream: two hs_place_db_add_device,
    a relocalisation query (the first query after an add: it uploads the walk order and waits for the stream inside the library) and a loop query (steady
    state: waits for nothing).  The adds have no output of their own: a vector that arrived late or early shows in the queries, which are perturbed
    copies of the added vectors.  -> dict(n_words, host=[(key, words, values)], steps=[Case])"""
    from place_cases import random_scene
    n_words, n_host, m_max, qm_max = 1000, 30, 64, 96
    scr, scd = random_scene(5, n_host + 2, n_words, erase=0.0), random_scene(6, n_host + 2, n_words, erase=0.0)
    host = scr["entries"][:n_host]
    keys = [e[0] for e in scr["entries"]]
    slot_of = {k: i for i, k in enumerate(keys)}
    n_slots = n_host + 2
    adds_r, adds_d = scr["entries"][n_host:], [(keys[n_host + i], e[1], e[2]) for i, e in enumerate(scd["entries"][n_host:])]
    refs = []
    for adds in (adds_r, adds_d):
        ref = ref_place.PlaceRecognizerRef(n_words)
        for k, w, v in host + adds:
            ref.add(k, w, v)
        refs.append(ref)
    steps = []
    for i in range(2):
        a, b = _padded_vec(adds_r[i][1], adds_r[i][2], m_max), _padded_vec(adds_d[i][1], adds_d[i][2], m_max)
        steps.append(Case("place_add", "slot %d" % (n_host + i), dict(word=pair(a[0], b[0]), value=pair(a[1], b[1]), m=pair(a[2], b[2])), {}, {},
                          args=dict(key=keys[n_host + i], m_max=m_max, slot=n_host + i)))
    rng = np.random.default_rng(7)
    tables = []
    for sc in (scr, scd):
        t = np.full((n_slots, 10), -1, np.int32)
        for i, k in enumerate(keys):
            row = [slot_of[x] for x in sc["neigh"][sc["entries"][i][0]] if x in slot_of][:10] if sc is scr else \
                  [int(x) for x in rng.choice(n_slots, int(rng.integers(0, 8)), replace=False) if x != i]
            t[i, :len(row)] = row
        tables.append(t)
    q1 = (_perturbed(rng, adds_r[0][1], n_words), _perturbed(rng, adds_d[1][1], n_words))
    q2 = (_perturbed(rng, adds_r[1][1], n_words), _perturbed(rng, adds_d[0][1], n_words))
    excl = [np.zeros(n_slots, np.uint8), np.zeros(n_slots, np.uint8)]
    excl[0][[3, 7]], excl[1][[1, 30]] = 1, 1
    steps.append(_query_case("first after add", False, slot_of, n_slots, refs, q1, tables, excl, 0.0, qm_max))
    steps.append(_query_case("steady state", True, slot_of, n_slots, refs, q2, tables, excl, float(np.float32(0.02)), qm_max))
    return dict(n_words=n_words, host=host, steps=steps)


# ---------------------------------------------------------------- the mixed chain
def _bow_of(desc):
    t = vocab_tree()["tree"]
    word, weight, node = ref_bow.bow_transform(t, desc, LEVELSUP)
    w, v = ref_place.bow_vector(word, weight)
    return (word, weight, node), (np.array(w, np.int32), np.array(v, np.float64))


def chain_scene(cap):
    """one frame through extract -> BoW transform -> BoW vector -> place add -> place query on ONE stream: every stage reads what the stage before it
    left on the device (`link`), only the image and the neighbour table come from the host.  The intermediate buffers start from the DECOY's valid
    results (`prefill`), so a stage that runs early reads valid counts and indices.  The database holds four host-added frames, one of them the other
    view of the real frame's stereo pair.  -> dict(n_words, host, steps=[Case with .link and .prefill])"""
    t = vocab_tree()["tree"]
    n_words = int((np.asarray(t["word_id"]) >= 0).sum())
    a, b, c = stereo_pair_ref(7), stereo_pair_ref(8), stereo_pair_ref(9)
    frames = [(a[0], a[2], a[3]), (b[0], b[2], b[3])]             # (image, keypoints, descriptors): real, decoy
    host = [(900 - 7 * i, *_bow_of(d)[1]) for i, d in enumerate((a[5], b[5], c[3], c[5]))]
    new_key, n_slots = 333, len(host) + 1
    slot_of = {k: i for i, (k, _, _) in enumerate(host)}
    slot_of[new_key] = len(host)
    stage = []                                                     # per frame: every stage's reference
    for img, k, d in frames:
        assert len(k) <= cap <= 16384
        (word, weight, node), (w, v) = _bow_of(d)
        ref = ref_place.PlaceRecognizerRef(n_words)
        for key, hw, hv in host:
            ref.add(key, hw, hv)
        ref.add(new_key, w, v)
        neigh = np.full((n_slots, 10), -1, np.int32)
        if img is frames[0][0]:
            neigh[0, :2], neigh[n_slots - 1, :1] = (1, n_slots - 1), (0,)
        else:
            neigh[1, :2], neigh[n_slots - 1, :1] = (2, n_slots - 1), (3,)
        key_of = {s: kk for kk, s in slot_of.items()}
        keys, det = ref.detect_reloc(w, v, {kk: [key_of[int(x)] for x in neigh[s] if x >= 0] for kk, s in slot_of.items()})
        stage.append(dict(img=img[None], kps=k, desc=d, n=np.array([len(k)], np.int32), word=word, weight=weight, node=node, out_word=w, out_value=v,
                          m=np.array([len(w)], np.int32), neigh=neigh, query=_query_expect(slot_of, n_slots, keys, det)))
    r, d = stage
    seg = lambda k: whole(r[k], d[k])
    pre = lambda *ks: {k: d[k] for k in ks}
    steps = [
        Case("extract_batch", "chain", dict(imgs=pair(r["img"], d["img"])), dict(kps=cap * KB, desc=cap * 32, n=4), {k: seg(k) for k in ("kps", "desc", "n")},
             args=dict(batch=1, w=W, h=H, cap=cap)),
        Case("bow_transform", "chain", {}, dict(word=4 * cap, weight=4 * cap, node=4 * cap), {k: seg(k) for k in ("word", "weight", "node")}, args=dict(n_max=cap)),
        Case("bow_vector", "chain", {}, dict(out_word=4 * cap, out_value=8 * cap, m=4), {k: seg(k) for k in ("out_word", "out_value", "m")}, args=dict(n_max=cap)),
        Case("place_add", "chain", {}, {}, {}, args=dict(key=new_key, m_max=cap, slot=n_slots - 1)),
        Case("place_query_reloc", "chain", dict(neigh=pair(r["neigh"], d["neigh"])), dict(cand=4 * n_slots, n_cand=4, words=4 * n_slots, score=4 * n_slots, acc=4 * n_slots, best=4 * n_slots),
             {k: whole(r["query"][k], d["query"][k]) for k in QUERY_OUT}, args=dict(qm_max=cap, slots=n_slots, min_score=0.0), primary=("words", "score")),
    ]
    links = [{}, dict(desc=(0, "desc"), n=(0, "n")), dict(word=(1, "word"), weight=(1, "weight"), n=(0, "n")), dict(word=(2, "out_word"), value=(2, "out_value"), m=(2, "m")),
             dict(qword=(2, "out_word"), qvalue=(2, "out_value"), qm=(2, "m"))]
    prefills = [pre("kps", "desc", "n"), pre("word", "weight", "node"), pre("out_word", "out_value", "m"), {}, {}]
    for s, l, p in zip(steps, links, prefills):
        s.link, s.prefill = l, p
    return dict(n_words=n_words, host=host, steps=steps)


# ---------------------------------------------------------------- every case, for tests/test_stream_order_cases.py
CPU_CAP = 1100                                                    # stands for hs_orb_max_keypoints() where no handle exists: above every count of the scenes


def single_cases(cap=CPU_CAP):
    return [landmark_case("small"), landmark_case("large"), kf_votes_case("lds"), kf_votes_case("global"), kf_redundancy_case(), local_keyframes_case(),
            local_points_case(), landmark_gather_case(), local_map_search_case(), extract_case(cap), extract_case(cap, seeds=(9, 10)), stereo_frontend_case(cap),
            stereo_match_case(), preprocess_case(), projection_case(False), projection_case(True), pose_edges_case(), pose_optimize_case(), knn2_case(),
            records_knn2_case(), records_bow_match_case(5), records_bow_match_case(4), bow_transform_case(900, (893, 860)), bow_transform_case(200, (200, 150)),
            bow_vector_case(5000, (4990, 4500)), bow_vector_case(300, (300, 280))]


def valid_table(T, which):
    """what the kernels trust of an observation table"""
    off, kf = T["T.lm_obs_offsets"][which], T["T.lm_obs_kf"][which]
    n_kf = len(T["T.kf_id"][which])
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(kf) == len(T["T.lm_obs_octave"][which])
    assert kf.min(initial=0) >= 0 and kf.max(initial=0) < n_kf
    for a, b in zip(off[:-1], off[1:]):
        assert (np.diff(kf[a:b]) > 0).all()                       # ascending slots per landmark
