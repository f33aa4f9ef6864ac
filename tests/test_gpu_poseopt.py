"""GPU: the pose-only optimisation — hs_pose_optimize(_device) and hs_pose_edges_device — against tests/ref_poseopt.py (pinned by
tests/test_poseopt_ref.py) through tests/golden/poseopt_cases.npz, which holds every case's inputs and the reference's outputs.

Exact on every edge of every case: the outlier flags, n_good, n_edges, rounds, status.  The pose: Tcw_d entry by entry within tau = 16 x the largest
deviation the reference shows against itself under 8 summation orders (stored in the golden file; the device differs from the reference by a
tree-shaped summation and its own sin / cos / sqrt, nothing larger), Tcw = float32(Tcw_d) of the device bit for bit and within 1 float ulp of the
reference's.  Through the C ABI host form, the Python method and the device form on a caller stream, with 0x55-filled outputs and guard bytes.

Beyond the cases: an edge list on a 16-byte boundary, the edge count read from the device (below 0, 0, 2, 3, above edge_cap), 70 problems in one
launch, and hs_pose_edges_device on synthetic frames of one to three 1024-keypoint chunks (P.edge_frame) with the chain on 2049 keypoints."""
import ctypes as C

import numpy as np
import pytest

import hipmem
import poseopt_cases as P
import ref_poseopt as R

pytestmark = pytest.mark.gpu

GUARD = 64
NAMES = sorted(P.SPECS)


@pytest.fixture(scope="module")
def golden():
    return P.load_golden()


@pytest.fixture(scope="module")
def opt(gpu):
    import hyslam_amd as HS
    return HS.Optimizer(extractor=HS.ORBExtractor(device=0))


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def dev(a):
    return hipmem.DevBuf.from_numpy(np.ascontiguousarray(a))


def dev_at(a, shift):
    """a copy of `a` at byte offset `shift` of a fresh allocation whose start is 32-byte aligned -> (buffer, device address of the copy)"""
    a = np.ascontiguousarray(a)
    b = hipmem.DevBuf(a.nbytes + shift, zero=False)
    assert b.ptr % 32 == 0
    if a.nbytes:
        hipmem._ok(hipmem.hip().hipMemcpy(b.ptr + shift, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")
    return b, b.ptr + shift


def out_buf(nbytes):
    b = hipmem.DevBuf(nbytes + GUARD)
    b.fill(0x55)
    return b


def read(buf, dtype, count):
    nbytes = np.dtype(dtype).itemsize * count
    raw = buf.to_numpy(np.uint8, nbytes + GUARD)
    assert (raw[nbytes:] == 0x55).all(), "bytes written behind the output"
    return raw[:nbytes].view(dtype).copy()


def problems(items):
    """items: (T, cam, edges) per problem -> (hs_pose_problem [Q], offsets int64 [Q + 1], edges)"""
    from hyslam_amd import _native as N
    prob = np.zeros(len(items), N.POSE_PROBLEM_DTYPE)
    for q, (T, cam, _) in enumerate(items):
        prob["Tcw"][q] = np.asarray(T, np.float32).reshape(16)
        for k, v in zip(("fx", "fy", "cx", "cy", "bf"), cam):
            prob[k][q] = v
    off = np.zeros(len(items) + 1, np.int64)
    off[1:] = np.cumsum([len(e) for _, _, e in items])
    lists = [np.ascontiguousarray(e, N.POSE_EDGE_DTYPE) for _, _, e in items]
    return prob, off, (np.concatenate(lists) if lists else np.zeros(0, N.POSE_EDGE_DTYPE))


def run_host(ex, items):
    """the C ABI host form on sentinel-filled outputs with guards -> (results, outlier)"""
    from hyslam_amd import _native as N
    prob, off, edges = problems(items)
    n, Q = len(edges), len(items)
    outlier = np.full(n + GUARD, 0x55, np.uint8)
    res = np.full(Q * N.POSE_RESULT_DTYPE.itemsize + GUARD, 0x55, np.uint8)
    N.check(ex._h, ex._lib.hs_pose_optimize(ex._h, Q, p(prob), p(off), p(edges), p(outlier), p(res)))
    assert (outlier[n:] == 0x55).all() and (res[Q * N.POSE_RESULT_DTYPE.itemsize:] == 0x55).all(), "bytes written behind the output"
    return res[:Q * N.POSE_RESULT_DTYPE.itemsize].view(N.POSE_RESULT_DTYPE).copy(), outlier[:n].copy()


def run_device(ex, items, stream, shift=0):
    """the device form with offsets; the edge list starts `shift` bytes behind a 32-byte boundary"""
    from hyslam_amd import _native as N
    prob, off, edges = problems(items)
    n, Q = len(edges), len(items)
    d_prob, d_off = dev(prob), dev(off)
    keep, edges_ptr = dev_at(edges, shift)
    d_out, d_res = out_buf(n), out_buf(Q * N.POSE_RESULT_DTYPE.itemsize)
    nwork = ex.pose_work_bytes(Q, n)
    work = out_buf(nwork)
    ex.pose_optimize_device(Q, d_prob.ptr, edges_ptr, d_out.ptr, d_res.ptr, d_edge_offsets=d_off.ptr, d_work=work.ptr if nwork else None, stream=stream.ptr)
    stream.synchronize()
    read(work, np.uint8, nwork)
    return read(d_res, N.POSE_RESULT_DTYPE, Q), read(d_out, np.uint8, n)


def item(golden, name):
    return golden[name + ".T"], golden[name + ".cam"], golden[name + ".edges"]


@pytest.mark.parametrize("name", NAMES)
def test_case_against_the_reference(opt, golden, name):
    ex, tau = opt._ex, float(golden["tau"])
    T, cam, edges = item(golden, name)
    res, outlier = run_host(ex, [(T, cam, edges)])
    r = res[0]
    g = lambda k: golden[name + "." + k]
    dev_d = float(np.abs(r["Tcw_d"].reshape(4, 4) - g("Tcw_d")).max())
    print("%s: |Tcw_d - reference| %.3e (tau %.3e); iterations %d / %d, trials %d / %d" % (name, dev_d, tau, r["lm_iterations"], int(g("lm_iterations")),
                                                                                           r["lm_trials"], int(g("lm_trials"))))
    assert np.array_equal(outlier, g("outlier")), "flags differ on edges %s" % np.nonzero(outlier != g("outlier"))[0][:10]
    assert [int(r[k]) for k in ("n_good", "n_edges", "rounds", "status")] == [int(g(k)) for k in ("n_good", "n_edges", "rounds", "status")]
    assert dev_d <= tau
    assert r["Tcw"].tobytes() == r["Tcw_d"].astype(np.float32).tobytes()
    assert np.abs(r["Tcw"].view(np.int32).astype(np.int64) - g("Tcw").reshape(16).view(np.int32).astype(np.int64)).max() <= 1
    if name in P.DIRECTED:                                        # the reference's path is the same under all 8 summation orders
        assert (int(r["lm_iterations"]), int(r["lm_trials"])) == (int(g("lm_iterations")), int(g("lm_trials")))
    # the device form on a caller stream and the Python method: the same bytes
    res_d, outlier_d = run_device(ex, [(T, cam, edges)], hipmem.Stream())
    assert res_d.tobytes() == res.tobytes() and outlier_d.tobytes() == outlier.tobytes()
    Tcw, flags, n_good = opt.PoseOptimization(T, cam, edges)
    assert Tcw.tobytes() == r["Tcw"].tobytes() and n_good == int(r["n_good"]) and len(flags) == int(edges["kp"].max()) + 1
    assert np.array_equal(flags[edges["kp"]], outlier) and int(flags.sum()) == int(outlier.sum())


@pytest.mark.parametrize("n", P.TOO_FEW)
def test_fewer_than_three_edges_run_nothing(opt, n):
    from hyslam_amd import _native as N
    T, cam, edges = P.too_few(n)
    for res, outlier in (run_host(opt._ex, [(T, cam, edges)]), run_device(opt._ex, [(T, cam, edges)], hipmem.Stream())):
        r = res[0]
        assert (outlier == 0x55).all() and len(outlier) == n      # not touched
        assert [int(r[k]) for k in ("n_edges", "n_good", "rounds", "lm_iterations", "lm_trials", "status")] == [n, 0, 0, 0, 0, N.HS_POSE_TOO_FEW]
        assert r["Tcw"].tobytes() == T.tobytes() and r["Tcw_d"].tobytes() == T.astype(np.float64).tobytes()
    Tcw, flags, n_good = opt.PoseOptimization(T, cam, edges)
    assert Tcw.tobytes() == T.tobytes() and n_good == 0 and not flags.any()


def batch_items(golden):
    T0, cam0, e0 = P.too_few(0)
    return [item(golden, P.BATCH[0]), (T0, cam0, e0), item(golden, P.BATCH[2])]


def test_same_call_twice_gives_the_same_bytes(opt, golden):
    for items in ([item(golden, "n1000")], batch_items(golden)):
        a, b = run_host(opt._ex, items), run_host(opt._ex, items)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        s = hipmem.Stream()
        a, b = run_device(opt._ex, items, s), run_device(opt._ex, items, s)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_batch_equals_its_problems_alone(opt, golden):
    ex, items = opt._ex, batch_items(golden)
    assert [len(e) for _, _, e in items] == [257, 0, 12]
    res, outlier = run_host(ex, items)
    res_d, outlier_d = run_device(ex, items, hipmem.Stream())
    assert res_d.tobytes() == res.tobytes() and outlier_d.tobytes() == outlier.tobytes()
    off = np.cumsum([0] + [len(e) for _, _, e in items])
    for q, it in enumerate(items):
        one, flags = run_host(ex, [it])
        assert one[0].tobytes() == res[q].tobytes() and flags.tobytes() == outlier[off[q]:off[q + 1]].tobytes()
    results, lists = opt.PoseOptimizationBatch([i[0] for i in items], [i[1] for i in items], [i[2] for i in items])
    assert results.tobytes() == res.tobytes() and np.array_equal(np.concatenate(lists), outlier)


def test_host_form_refuses_bad_offsets_and_leaves_outputs_alone(opt, golden):
    from hyslam_amd import _native as N
    ex = opt._ex
    prob, off, edges = problems(batch_items(golden))
    for bad in ([0, 257, 200, 269], [-1, 257, 257, 269]):
        outlier = np.full(len(edges), 0x55, np.uint8)
        res = np.full(3 * N.POSE_RESULT_DTYPE.itemsize, 0x55, np.uint8)
        b = np.array(bad, np.int64)
        assert ex._lib.hs_pose_optimize(ex._h, 3, p(prob), p(b), p(edges), p(outlier), p(res)) == N.HS_ERR_INVALID
        assert (outlier == 0x55).all() and (res == 0x55).all()
    d = out_buf(64)
    for offsets, n_edges, Q in ((None, None, 1), (d.ptr, d.ptr, 1), (None, d.ptr, 2)):      # exactly one of the two; d_n_edges needs Q == 1
        assert ex._lib.hs_pose_optimize_device(ex._h, Q, d.ptr, offsets, n_edges, 4, d.ptr, d.ptr, d.ptr, None, None) == N.HS_ERR_INVALID
    read(d, np.uint8, 64)


@pytest.fixture(scope="module")
def frame_scene():
    """a 640 x 480 stereo frame, landmarks around it, and for every keypoint the landmark that projects nearest to it (within 2 px), with entries that
    are -1, negative otherwise, L and beyond"""
    import scenes
    from hyslam_amd import _native as N
    sc = scenes.projection_scene(83, 640, 480, nfeat=300, copies=2)
    fa, lms = sc["frame_args"], np.ascontiguousarray(sc["lms"], N.LM_DTYPE)
    Rcw, tcw = np.asarray(fa["Rcw"], np.float64).reshape(3, 3), np.asarray(fa["tcw"], np.float64)
    Pc = lms["pos"].astype(np.float64) @ Rcw.T + tcw
    z = np.where(Pc[:, 2] > 0.1, Pc[:, 2], np.inf)
    uv = np.stack([fa["fx"] * Pc[:, 0] / z + fa["cx"], fa["fy"] * Pc[:, 1] / z + fa["cy"]], 1)
    kps = fa["kps"]
    d2 = (kps["x"][:, None] - uv[None, :, 0]) ** 2 + (kps["y"][:, None] - uv[None, :, 1]) ** 2
    near = d2.argmin(1)
    kp_lm = np.where(d2[np.arange(len(kps)), near] < 4.0, near, -1).astype(np.int32)
    held = np.nonzero(kp_lm >= 0)[0]
    assert len(held) > 150 and (np.asarray(fa["uR"])[held] < 0).any() and (np.asarray(fa["uR"])[held] >= 0).any()
    kp_lm[held[3]], kp_lm[held[10]], kp_lm[held[20]], kp_lm[held[-1]] = len(lms), len(lms) + 7, -7, -1
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = np.asarray(fa["Rcw"], np.float32).reshape(3, 3), np.asarray(fa["tcw"], np.float32)
    cam = np.array([fa["fx"], fa["fy"], fa["cx"], fa["cy"], fa["mbf"]], np.float32)
    return dict(fa=fa, lms=lms, kp_lm=kp_lm, T=T, cam=cam)


def device_frame(fa):
    import oracle
    from hyslam_amd import _native as N
    Fh, keep = oracle.make_frame_view(N.FrameView, **fa)
    bufs = [dev(np.ascontiguousarray(fa["kps"], N.KP_DTYPE)), dev(np.ascontiguousarray(fa["uR"], np.float32))]
    Fd = N.FrameView.from_buffer_copy(Fh)
    Fd.kps, Fd.uR, Fd.desc, Fd.kp_lm_obs = bufs[0].ptr, bufs[1].ptr, None, None
    return Fd, bufs


def test_edges_device_and_the_chain(opt, frame_scene):
    from hyslam_amd import _native as N
    ex, sc = opt._ex, frame_scene
    fa, lms, kp_lm = sc["fa"], sc["lms"], sc["kp_lm"]
    want, count = R.gather_edges(fa["kps"], fa["uR"], kp_lm, lms["pos"], size_ref=31.0, sigma_ref=1.0)
    assert count == len(want) > 100 and (np.diff(want["kp"]) > 0).all()
    assert np.array_equal(want, opt.pose_edges(fa["kps"], fa["uR"], kp_lm, lms))          # the Python gather is the same list
    Fd, keep = device_frame(fa)
    d_lms, d_kp_lm = dev(lms), dev(kp_lm)
    stream = hipmem.Stream()
    esz = N.POSE_EDGE_DTYPE.itemsize
    for cap in (count - 37, count, count + 50, 0):
        d_edges, d_n = out_buf(cap * esz), out_buf(4)
        ex.pose_edges_device(Fd, d_lms.ptr, len(lms), d_kp_lm.ptr, d_edges.ptr, cap, d_n.ptr, sigma_ref=1.0, stream=stream.ptr)
        stream.synchronize()
        assert int(read(d_n, np.int32, 1)[0]) == count             # the full count, whatever cap
        got = read(d_edges, np.uint8, cap * esz)
        k = min(cap, count)
        assert got[:k * esz].tobytes() == want[:k].tobytes() and (got[k * esz:] == 0x55).all()
    # the chain: edges -> optimisation on one stream, the count never leaving the device; against the host form fed the same edges
    cap = count + 50
    d_edges, d_n = out_buf(cap * esz), out_buf(4)
    prob, _, _ = problems([(sc["T"], sc["cam"], want)])
    d_prob, d_out, d_res = dev(prob), out_buf(cap), out_buf(N.POSE_RESULT_DTYPE.itemsize)
    ex.pose_edges_device(Fd, d_lms.ptr, len(lms), d_kp_lm.ptr, d_edges.ptr, cap, d_n.ptr, sigma_ref=1.0, stream=stream.ptr)
    ex.pose_optimize_device(1, d_prob.ptr, d_edges.ptr, d_out.ptr, d_res.ptr, d_n_edges=d_n.ptr, edge_cap=cap, stream=stream.ptr)
    stream.synchronize()
    res, outlier = run_host(ex, [(sc["T"], sc["cam"], want)])
    flags = read(d_out, np.uint8, cap)
    assert read(d_res, N.POSE_RESULT_DTYPE, 1).tobytes() == res.tobytes() and flags[:count].tobytes() == outlier.tobytes() and (flags[count:] == 0x55).all()
    assert int(res["status"][0]) == N.HS_POSE_OK and int(res["rounds"][0]) == 4 and 0 < int(res["n_good"][0]) <= count
    # a cap below the count truncates the problem as well
    small = count - 37
    d_out2, d_res2 = out_buf(small), out_buf(N.POSE_RESULT_DTYPE.itemsize)
    ex.pose_optimize_device(1, d_prob.ptr, d_edges.ptr, d_out2.ptr, d_res2.ptr, d_n_edges=d_n.ptr, edge_cap=small, stream=stream.ptr)
    stream.synchronize()
    res2, outlier2 = run_host(ex, [(sc["T"], sc["cam"], want[:small])])
    assert read(d_res2, N.POSE_RESULT_DTYPE, 1).tobytes() == res2.tobytes() and read(d_out2, np.uint8, small).tobytes() == outlier2.tobytes()


def test_edge_list_on_a_16_byte_boundary(opt, golden):
    """hs_pose_optimize_device asks for 16-byte alignment of d_edges and the kernel reads a 32-byte edge as two 16-byte halves: a list that starts
    16 bytes behind a 32-byte boundary gives the bytes of the aligned run; one at offset 4 is refused before anything is launched"""
    from hyslam_amd import _native as N
    ex, it = opt._ex, item(golden, "n257")
    stream = hipmem.Stream()
    res, outlier = run_device(ex, [it], stream)
    res16, outlier16 = run_device(ex, [it], stream, shift=16)
    assert res16.tobytes() == res.tobytes() and outlier16.tobytes() == outlier.tobytes()
    assert int(res["status"][0]) == N.HS_POSE_OK and int(res["n_edges"][0]) == 257
    prob, off, edges = problems([it])
    d_prob, d_off = dev(prob), dev(off)
    keep, edges_ptr = dev_at(edges, 4)
    d_out, d_res = out_buf(len(edges)), out_buf(N.POSE_RESULT_DTYPE.itemsize)
    assert ex._lib.hs_pose_optimize_device(ex._h, 1, d_prob.ptr, d_off.ptr, None, 0, edges_ptr, d_out.ptr, d_res.ptr, None, stream.ptr) == N.HS_ERR_INVALID
    stream.synchronize()
    assert (read(d_out, np.uint8, len(edges)) == 0x55).all() and (read(d_res, np.uint8, N.POSE_RESULT_DTYPE.itemsize) == 0x55).all()


def test_edge_count_read_from_the_device(opt, golden):
    """d_n_edges: the kernel clamps the count it reads to 0 .. edge_cap.  Below 3 nothing is optimised and no flag is written; from 3 on the
    problem is the prefix of that length"""
    from hyslam_amd import _native as N
    ex = opt._ex
    T, cam, edges = item(golden, "n257")
    prob, _, _ = problems([(T, cam, edges)])
    d_prob, d_edges = dev(prob), dev(np.ascontiguousarray(edges, N.POSE_EDGE_DTYPE))
    stream, cap = hipmem.Stream(), 100
    for value in (-5, 0, 2, 3, cap + 1):
        n = min(max(value, 0), cap)
        d_n, d_out, d_res = dev(np.array([value], np.int32)), out_buf(len(edges)), out_buf(N.POSE_RESULT_DTYPE.itemsize)
        ex.pose_optimize_device(1, d_prob.ptr, d_edges.ptr, d_out.ptr, d_res.ptr, d_n_edges=d_n.ptr, edge_cap=cap, stream=stream.ptr)
        stream.synchronize()
        assert int(d_n.to_numpy(np.int32, 1)[0]) == value
        r, flags = read(d_res, N.POSE_RESULT_DTYPE, 1), read(d_out, np.uint8, len(edges))
        assert (flags[n:] == 0x55).all()
        if n < 3:
            assert (flags == 0x55).all()
            assert [int(r[k][0]) for k in ("n_edges", "n_good", "rounds", "lm_iterations", "lm_trials", "status")] == [n, 0, 0, 0, 0, N.HS_POSE_TOO_FEW]
            assert r["Tcw"][0].tobytes() == T.tobytes() and r["Tcw_d"][0].tobytes() == T.astype(np.float64).tobytes()
        else:
            res, outlier = run_host(ex, [(T, cam, edges[:n])])
            assert r.tobytes() == res.tobytes() and flags[:n].tobytes() == outlier.tobytes()
            assert int(r["status"][0]) == N.HS_POSE_OK and int(r["n_edges"][0]) == n


def test_seventy_problems_in_one_launch(opt, golden):
    """Q = 70: every golden case once and 29 of them a second time, in a seeded order, with two problems without edges and one of 2 edges in
    between.  Each result and each range of flags is that of the problem run alone; the host and the device form agree, and a second call too"""
    from hyslam_amd import _native as N
    ex = opt._ex
    rng = np.random.default_rng(70)
    names = [str(x) for x in rng.permutation(NAMES)] + [str(x) for x in rng.permutation(NAMES)[:67 - len(NAMES)]]
    items = [item(golden, name) for name in names]
    for at, n in ((9, 0), (30, 2), (55, 0)):
        T, cam, e = P.too_few(n)
        items.insert(at, (T, cam, e))
        names.insert(at, "too_few_%d" % n)
    assert len(items) == 70 and [len(items[i][2]) for i in (9, 30, 55)] == [0, 2, 0]
    res, outlier = run_host(ex, items)
    again = run_host(ex, items)
    assert again[0].tobytes() == res.tobytes() and again[1].tobytes() == outlier.tobytes()
    stream = hipmem.Stream()
    for _ in range(2):
        res_d, outlier_d = run_device(ex, items, stream)
        assert res_d.tobytes() == res.tobytes() and outlier_d.tobytes() == outlier.tobytes()
    off = np.cumsum([0] + [len(e) for _, _, e in items])
    alone = {}
    for q, name in enumerate(names):
        if name not in alone:
            alone[name] = run_host(ex, [items[q]])
        one, flags = alone[name]
        assert one[0].tobytes() == res[q].tobytes() and flags.tobytes() == outlier[off[q]:off[q + 1]].tobytes(), (q, name)
    assert sorted(int(x) for x in np.unique(res["status"])) == [N.HS_POSE_OK, N.HS_POSE_TOO_FEW]


class EdgeGather:
    """hs_pose_edges_device on arrays uploaded once: run(cap) -> (count on the device, the bytes of a 0x55-filled buffer of cap edges)"""

    def __init__(self, ex, stream, kps, uR, kp_lm, lm_pos, size_ref=31.0, sigma_ref=1.0):
        from hyslam_amd import _native as N
        self.ex, self.stream, self.sigma_ref, self.L = ex, stream, sigma_ref, len(lm_pos)
        lms = np.zeros(len(lm_pos), N.LM_DTYPE)
        lms["pos"] = lm_pos
        n = len(kps)
        self.d_kps = dev(np.ascontiguousarray(kps, N.KP_DTYPE)) if n else None
        self.d_uR = dev(np.ascontiguousarray(uR, np.float32)) if n and uR is not None else None
        self.d_kp_lm = dev(np.ascontiguousarray(kp_lm, np.int32)) if n else None
        self.d_lms = dev(lms) if len(lms) else None
        self.F = N.FrameView()
        self.F.n, self.F.size_ref = n, size_ref
        self.F.kps, self.F.uR = (b.ptr if b is not None else None for b in (self.d_kps, self.d_uR))
        self.F.desc, self.F.kp_lm_obs = None, None

    def launch(self, d_edges, cap, d_n):
        g = lambda b: b.ptr if b is not None else None
        self.ex.pose_edges_device(self.F, g(self.d_lms), self.L, g(self.d_kp_lm), d_edges.ptr, cap, d_n.ptr, sigma_ref=self.sigma_ref, stream=self.stream.ptr)

    def run(self, cap):
        from hyslam_amd import _native as N
        d_edges, d_n = out_buf(cap * N.POSE_EDGE_DTYPE.itemsize), out_buf(4)
        self.launch(d_edges, cap, d_n)
        self.stream.synchronize()
        return int(read(d_n, np.int32, 1)[0]), read(d_edges, np.uint8, cap * N.POSE_EDGE_DTYPE.itemsize)


def check_gather(ex, stream, f, caps, size_ref=31.0, sigma_ref=1.0, no_uR=False):
    """every cap: the full count on the device, the first min(cap, count) edges those of the reference byte for byte, the rest of the buffer and
    the guard (read()) as they were filled"""
    uR = np.full(len(f["kps"]), -1.0, np.float32) if no_uR else f["uR"]
    want, count = R.gather_edges(f["kps"], uR, f["kp_lm"], f["lm_pos"], size_ref=size_ref, sigma_ref=sigma_ref)
    g = EdgeGather(ex, stream, f["kps"], None if no_uR else f["uR"], f["kp_lm"], f["lm_pos"], size_ref, sigma_ref)
    esz = want.dtype.itemsize
    for cap in caps(count):
        got_count, got = g.run(cap)
        k = min(cap, count)
        assert got_count == count, (cap, got_count, count)
        assert got[:k * esz].tobytes() == want[:k].tobytes(), "cap %d: first differing edge %d" % (
            cap, int(np.nonzero((got[:k * esz].reshape(k, esz) != want[:k].view(np.uint8).reshape(k, esz)).any(1))[0][0]))
        assert (got[k * esz:] == 0x55).all(), cap
    return want, count


@pytest.mark.parametrize("n", P.EDGE_FRAME_SIZES)
def test_edges_device_beyond_one_chunk(opt, n):
    """k_pose_edges walks the keypoints in chunks of 1024 with a running base: keypoint counts at and around one and two chunks, lists that are
    sparse, that leave a whole chunk empty and that hold every keypoint, and a cap of 0, inside the first chunk, at the base of the second (and
    third) chunk, inside the second chunk, at the count and above it"""
    ex, stream = opt._ex, hipmem.Stream()
    for variant in P.EDGE_FRAME_VARIANTS:
        f = P.edge_frame(n, variant)
        held = (f["kp_lm"] >= 0) & (f["kp_lm"] < P.EDGE_FRAME_L)
        bases = [int(held[:c].sum()) for c in range(P.EDGE_CHUNK, n, P.EDGE_CHUNK)]       # the running base where each later chunk starts
        caps = lambda count: sorted(set(c for c in [0, 300] + bases + [b + 5 for b in bases] + [count, count + 50] if c >= 0))
        want, count = check_gather(ex, stream, f, caps)
        assert count == int(held.sum())
        if variant == "sparse" and n > P.EDGE_CHUNK:
            assert held[P.EDGE_CHUNK - 1] and held[P.EDGE_CHUNK] and 0 < bases[0] < count
        if variant == "gap" and n > P.EDGE_CHUNK:
            assert any(not held[c:c + P.EDGE_CHUNK].any() for c in range(0, n, P.EDGE_CHUNK)) and count > 0
        if variant == "all":
            assert count == n


def test_edges_device_fields_and_empty_inputs(opt):
    from hyslam_amd import _native as N
    ex, stream = opt._ex, hipmem.Stream()
    caps = lambda count: [count + 3]
    f = P.edge_frame(2049, "sparse")
    want, count = check_gather(ex, stream, f, caps, no_uR=True)                               # F.uR == NULL: every edge is mono
    assert count > 900 and (want["ur"] == -1.0).all()
    want, _ = check_gather(ex, stream, f, caps, size_ref=24.5, sigma_ref=1.7)               # the weight is float32(1 / (sigma_ref * (s * s))), bit for bit
    s = f["kps"]["size"][want["kp"]] / np.float32(24.5)
    assert (want["inv_sigma2"] != np.float32(1.0) / ((np.float32(1.7) * s) * s)).any()       # the order of the products is visible in these values
    f["kps"]["size"][P.EDGE_CHUNK] = np.inf                                                   # a keypoint of infinite size: weight 0
    want, _ = check_gather(ex, stream, f, caps)
    assert want["inv_sigma2"][want["kp"] == P.EDGE_CHUNK].tobytes() == np.float32(0.0).tobytes()
    empty = {k: v[:0] if k != "lm_pos" else v for k, v in P.edge_frame(1023, "all").items()}
    for frame in (empty, dict(P.edge_frame(1025, "all"), lm_pos=np.zeros((0, 3), np.float32))):   # F.n = 0; L = 0
        _, count = check_gather(ex, stream, frame, lambda count: [0, 8])
        assert count == 0


def test_chain_of_2049_keypoints(opt):
    """hs_pose_edges_device -> hs_pose_optimize_device with d_n_edges on one stream, the count never leaving the device, on a posed frame of 2049
    keypoints (P.chain_problem; tests/test_poseopt_ref.py qualifies it): the bytes of the host form fed the reference's list"""
    from hyslam_amd import _native as N
    ex, stream, c = opt._ex, hipmem.Stream(), P.chain_problem()
    want, count = R.gather_edges(c["kps"], c["uR"], c["kp_lm"], c["lm_pos"])
    assert count == P.CHAIN_N and want.tobytes() == c["edges"].tobytes()
    g = EdgeGather(ex, stream, c["kps"], c["uR"], c["kp_lm"], c["lm_pos"])
    cap = count + 50
    d_edges, d_n = out_buf(cap * N.POSE_EDGE_DTYPE.itemsize), out_buf(4)
    prob, _, _ = problems([(c["T"], c["cam"], want)])
    d_prob, d_out, d_res = dev(prob), out_buf(cap), out_buf(N.POSE_RESULT_DTYPE.itemsize)
    g.launch(d_edges, cap, d_n)
    ex.pose_optimize_device(1, d_prob.ptr, d_edges.ptr, d_out.ptr, d_res.ptr, d_n_edges=d_n.ptr, edge_cap=cap, stream=stream.ptr)
    stream.synchronize()
    res, outlier = run_host(ex, [(c["T"], c["cam"], want)])
    flags = read(d_out, np.uint8, cap)
    assert read(d_res, N.POSE_RESULT_DTYPE, 1).tobytes() == res.tobytes() and flags[:count].tobytes() == outlier.tobytes() and (flags[count:] == 0x55).all()
    assert read(d_edges, np.uint8, cap * N.POSE_EDGE_DTYPE.itemsize)[:count * N.POSE_EDGE_DTYPE.itemsize].tobytes() == want.tobytes()
    assert int(res["status"][0]) == N.HS_POSE_OK and int(res["rounds"][0]) == 4 and int(res["n_edges"][0]) == count
    assert 0.7 * count < int(res["n_good"][0]) < count                                        # 15 % gross outliers


def test_nonfinite_input_terminates_inside_its_outputs(opt):
    """one of 65 points lies in the camera's plane at the start pose (z = 0): only termination and bounds are asserted, no values"""
    from hyslam_amd import _native as N
    rng = np.random.default_rng(3)
    n = 65
    fx, fy, cx, cy, bf = P.CAM
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1, 1, n), rng.uniform(2, 25, n)], 1)
    e = np.zeros(n, R.EDGE_DTYPE)
    e["Xw"] = X
    e["u"], e["v"] = fx * X[:, 0] / X[:, 2] + cx + rng.normal(0, 0.5, n), fy * X[:, 1] / X[:, 2] + cy + rng.normal(0, 0.5, n)
    e["ur"] = np.where(np.arange(n) % 2 == 0, e["u"] - bf / X[:, 2], -1.0)
    e["inv_sigma2"], e["kp"] = 1.0, np.arange(n)
    for k in (6, 7):                                              # a stereo and a mono edge
        e["Xw"][k] = (0.3, 0.2, 0.0)
    T, cam = np.eye(4, dtype=np.float32), np.array(P.CAM, np.float32)
    for res, outlier in (run_host(opt._ex, [(T, cam, e)]), run_device(opt._ex, [(T, cam, e)], hipmem.Stream())):
        r = res[0]
        print("non-finite input: status %d, rounds %d, iterations %d, trials %d, n_good %d" % (r["status"], r["rounds"], r["lm_iterations"], r["lm_trials"], r["n_good"]))
        assert int(r["status"]) in (N.HS_POSE_OK, N.HS_POSE_NONFINITE) and int(r["n_edges"]) == n and 1 <= int(r["rounds"]) <= 4
        assert 0 <= int(r["n_good"]) <= n and int(r["lm_iterations"]) <= 40 and int(r["lm_trials"]) <= 400 and (outlier <= 1).all()
