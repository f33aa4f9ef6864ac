"""The jobs of tests/test_gpu_concurrent_handles.py: one entry-point call each, by role (the host system's threads: image
processing, tracking, mapping, loop closing), with the result the references give for it.  Nothing here needs a device to be imported or to compute an
expected value; tests/test_concurrent_jobs.py holds that on the CPU.

A Job has a name, a role, expected() -> what the references give (computed once per process: ref_*.py, the oracle, pyref and the case tables the
single-call tests already use, never the device) and make(env) -> f.  make binds handles and device buffers of the calling worker's own (env: an Env,
created on the worker's thread); f() makes the call and returns None, or a short text naming the first thing that differs.  The comparison is the one
of the job's single-call test: bit-exact everywhere, Tcw_d within chain_compare.TAU.

Three kinds of job:
  case jobs     a stream_order_cases.Case (the `*_device` entry point on the worker's caller stream, late-input pairs of which only the real half is
                used here): inputs uploaded once, outputs refilled with 0x55 before every call, every defined byte compared
  method jobs   a method of the Python mirror on host arrays, compared as its own GPU test compares it
  host twins    the host-pointer form of a call whose case job runs by device pointers, on the same real inputs and the same expected bytes: the
                staging through the handle's scratch arena and pinned buffers runs under concurrency too"""
import functools

import numpy as np

ROLES = ("images", "tracking", "mapping", "loop")
FILL = 0x55


class Env:
    """what one worker owns: a caller stream, and one handle per extractor configuration it asks for"""

    def __init__(self):
        import hipmem
        import hyslam_amd as HS
        self.HS, self.stream, self._handles, self.keep = HS, hipmem.Stream(non_blocking=True), {}, []

    def extractor(self, nfeatures=1000, scale=1.2, nlevels=8, n_cells=30, fast_threshold=20, blur_taps=None, tag=""):
        key = (nfeatures, scale, nlevels, n_cells, fast_threshold, tag)
        if key not in self._handles:
            st = self.HS.FeatureExtractorSettings(nFeatures=nfeatures, fScaleFactor=scale, nLevels=nlevels, N_CELLS=n_cells)
            self._handles[key] = self.HS.ORBExtractor(st, blur_taps=blur_taps, fast_threshold=fast_threshold)
        return self._handles[key]

    def close(self):
        self.keep = []
        for ex in self._handles.values():
            ex.close()
        self._handles = {}


class Job:
    def __init__(self, role, name, expected, make):
        assert role in ROLES
        self.role, self.name, self.expected, self.make = role, name, expected if hasattr(expected, "cache_info") else functools.lru_cache(maxsize=None)(expected), make

    def __repr__(self):
        return "%s/%s" % (self.role, self.name)


def asserted(f):
    """f() compares with assert, as the single-call tests do: an AssertionError is the job's outcome"""
    @functools.wraps(f)
    def g(*a, **kw):
        try:
            return f(*a, **kw)
        except AssertionError as e:
            return "differs: %s" % (str(e)[:240] or "assertion")
    return g


def _raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


# ---------------------------------------------------------------- case jobs
def case_mismatch(case, got):
    """the first defined segment of `got` ({output: bytes}) that is not the reference's bytes for the real inputs, or None"""
    for k, segs in case.expect.items():
        for off, real, _ in segs:
            r = _raw(real)
            g = got[k][off:off + r.nbytes]
            if g.tobytes() != r.tobytes():
                what = "the fill" if len(g) and (g == FILL).all() else "other bytes"
                return "%r: %s at byte %d holds %s" % (case, k, off, what)
    return None


def bind_case(case, ex, stream, voc=None, db=None):
    """the call of `case` on handle `ex` and caller stream `stream`, its real inputs uploaded into buffers of its own -> f"""
    import hipmem
    from test_gpu_stream_order import step
    st = step(case, ex, voc=voc, db=db)
    D = hipmem.DevBuf
    bufs = {k: D.from_numpy(_raw(real)) for k, (real, _) in case.inputs.items()}
    for k, n in list(case.outputs.items()) + list(st.work.items()):
        bufs[k] = D(n, zero=False)
        bufs[k].fill(FILL)
    ptrs = {k: b.ptr for k, b in bufs.items()}

    @asserted
    def f():
        for k, n in case.outputs.items():
            hipmem.memset_async(bufs[k].ptr, FILL, n, stream)
        st.call(ptrs, stream.ptr)
        stream.synchronize()
        got = {k: bufs[k].read_after(stream, count=n) for k, n in case.outputs.items()}
        bad = case_mismatch(case, got)
        if bad is None and st.check is not None:
            st.check(got, "real")
        return bad
    f.bufs = bufs
    return f


def case_job(role, name, build, nfeatures=None):
    """build() -> Case (cached); the handle is the worker's stream_order_cases.NF one"""
    def make(env):
        import stream_order_cases as S
        return bind_case(job.expected(), env.extractor(nfeatures or S.NF), env.stream)
    job = Job(role, name, build, make)
    return job


def _S():
    import stream_order_cases as S
    return S


def extract_device_job():
    """hs_orb_extract_batch_device, 2 x 640 x 480 on a handle of its own; the row stride of the outputs is the handle's max_keypoints()"""
    def make(env):
        S = _S()
        ex = env.extractor(S.NF, tag="extract_batch_device")
        ex.reserve(S.W, S.H, 2)
        return bind_case(S.extract_case(ex.max_keypoints()), ex, env.stream)
    return Job("images", "extract_batch_device 2x640x480", lambda: _S().extract_case(_S().CPU_CAP), make)


def stereo_frontend_device_job():
    def make(env):
        S = _S()
        ex = env.extractor(S.NF, tag="stereo_frontend_device")
        ex.reserve(S.W, S.H, 4)
        return bind_case(S.stereo_frontend_case(ex.max_keypoints()), ex, env.stream)
    return Job("images", "stereo_frontend_batch_device 2 pairs 640x480", lambda: _S().stereo_frontend_case(_S().CPU_CAP), make)


def bow_transform_job(n_max, counts):
    """hs_bow_transform_device on a device vocabulary of the worker's own"""
    def make(env):
        S = _S()
        import scenes
        from hyslam_amd import _native as N
        from hyslam_amd import distributed as D
        ex = env.extractor(S.NF)
        e = S.vocab_tree()
        voc = D.DeviceVocabulary(ex, scenes.tree_struct(N.VocabTree, e["tree"]), S.LEVELSUP, keepalive=e["tree"])
        env.keep.append(voc)
        return bind_case(job.expected(), ex, env.stream, voc=voc)
    job = Job("loop", "bow_transform_device n_max %d" % n_max, lambda: _S().bow_transform_case(n_max, counts), make)
    return job


# ---------------------------------------------------------------- method jobs: images
def extract_job(name):
    """ORBExtractor.__call__ on a directed frame of tests/extract_cases.py against ref_extract"""
    @functools.lru_cache(maxsize=None)
    def expected():
        import extract_cases as X
        return X.reference(name)[:2]

    def make(env):
        import extract_cases as X
        from _extract_edge_check import assert_features
        c = X.CASES[name]
        ex = env.extractor(**X.settings_of(c))
        rk, rd = expected()

        @asserted
        def f():
            gk, gd = ex(c["img"])
            assert_features(name, gk, gd, rk, rd)
        return f
    return Job("images", "extract %s" % name, expected, make)


def extract_batch_job():
    @functools.lru_cache(maxsize=None)
    def expected():
        import extract_cases as X
        return [X.reference(n)[:2] for n in X.BATCH_273x225]

    def make(env):
        import extract_cases as X
        from _extract_edge_check import assert_features
        ex = env.extractor(tag="batch", **X.GEOM)
        imgs, want = [X.CASES[n]["img"] for n in X.BATCH_273x225], expected()

        @asserted
        def f():
            ks, ds = ex.extract_batch(imgs)
            for n, gk, gd, (rk, rd) in zip(X.BATCH_273x225, ks, ds, want):
                assert_features(n, gk, gd, rk, rd)
        return f
    return Job("images", "extract_batch BATCH_273x225", expected, make)


def _stereo_settings():
    import extract_cases as X
    kw = X.STEREO
    return dict(nfeatures=kw["nfeatures"], scale=kw["scale"], nlevels=kw["nlevels"], n_cells=kw["n_cells"])


def ticket_job():
    """the 320 x 240 stereo front end through a ticket (hs_orb_submit_batch / hs_orb_wait) against ref_extract.stereo_frontend"""
    @functools.lru_cache(maxsize=None)
    def expected():
        import extract_cases as X
        return X.stereo_reference(0)

    def make(env):
        import extract_cases as X
        from _extract_edge_check import assert_features
        ex = env.extractor(tag="ticket", **_stereo_settings())
        kw = X.STEREO
        sp = env.HS.stereo_params(env.HS.Camera(fx=kw["fx"], mbf=kw["mbf"], mnMaxY=float(kw["n_rows"])))
        L, R = X.stereo_pairs()[0]
        rkL, rdL, rkR, rdR, ru, rz = expected()

        @asserted
        def f():
            n, k, d, u, z = ex.wait(ex.submit_batch([L, R], sp))
            assert_features("left", k[0, :n[0]], d[0, :n[0]], rkL, rdL)
            assert_features("right", k[1, :n[1]], d[1, :n[1]], rkR, rdR)
            assert u[0, :n[0]].tobytes() == ru.tobytes() and z[0, :n[0]].tobytes() == rz.tobytes(), "uRight / depth"
        return f
    return Job("images", "stereo ticket 320x240", expected, make)


@functools.lru_cache(maxsize=None)
def published_scene():
    """the left frame of the 320 x 240 pair as the reference extracts it, 300 landmarks around its keypoints (scenes._area_landmarks), and the oracle's
    local-map search over them: what a search on the published extraction of that frame must return"""
    import extract_cases as X
    import oracle
    import scenes
    f32 = np.float32
    kl, dl = X.stereo_reference(0)[:2]
    rng = np.random.default_rng(17)
    n = len(kl)
    assert n > 100
    fa = dict(Rcw=np.eye(3, dtype=f32), tcw=np.zeros(3, f32), fx=260.0, fy=260.0, cx=160.0, cy=120.0, mbf=26.0, sensor=1, bounds=(0.0, 320.0, 0.0, 240.0),
              kps=kl, desc=dl, uR=(kl["x"] - rng.uniform(1, 20, n)).astype(f32), kp_lm_obs=rng.integers(-1, 3, n).astype(np.int32), size_ref=31.0)
    L = 300
    lms = scenes._area_landmarks(rng, fa, rng.integers(0, n, L), rng.choice([0, 3, 20], L))
    Fo, keep = oracle.make_frame_view(oracle.FrameView, **fa)
    oi, od, on = oracle.search_by_projection(Fo, lms, oracle.ProjParams(5.0, 100.0, 0.8, 0.5, 1.5, 1, 1, 0))
    assert on > 30
    return dict(fa=fa, lms=lms, want=(oi, od, on), images=X.stereo_pairs()[0])


def publish_job(require_hit=False):
    """extract with publish, find the frame by its keypoints, search it by token (FeatureMatcher falls back to host pointers when the cache refuses:
    another worker that published the same keypoints may own the slot that was found and release it under way), release"""
    def make(env):
        import oracle
        from _extract_edge_check import assert_features
        from hyslam_amd import _native as N
        sc = published_scene()
        ex = env.extractor(tag="publish", **_stereo_settings())
        m = env.HS.FeatureMatcher(env.HS.FeatureMatcherSettings(nnratio=0.8), ex)
        Fg, keep = oracle.make_frame_view(N.FrameView, **sc["fa"])
        oi, od, on = sc["want"]
        hits = []

        @asserted
        def f():
            (kl, _), (dl, _) = ex.extract_batch(list(sc["images"]), publish=True)
            try:
                assert_features("published left", kl, dl, sc["fa"]["kps"], sc["fa"]["desc"])
                assert all(ex.last_frame_tokens), "no token"
                gi, gd, gn = m.SearchByProjection(Fg, sc["lms"], 5.0)
                hits.append(m.frame_on_device)
                assert not require_hit or m.frame_on_device, "the published frame was not found on the device"
                assert np.array_equal(gi, oi) and np.array_equal(gd, od) and gn == on, "token search"
            finally:
                for t in ex.last_frame_tokens:
                    ex.release_frame(t)
        f.hits, f.keep = hits, keep
        return f
    return Job("images", "publish, find, search by token 320x240", lambda: published_scene()["want"], make)


# ---------------------------------------------------------------- method jobs: tracking
def track_frame_job(name):
    """hs_track_frame_device on a directed case of tests/track_cases.py in fresh buffers per call (tests/test_gpu_track.py's Chain), against ref_track"""
    @functools.lru_cache(maxsize=None)
    def expected():
        import track_cases as TC
        return TC.directed(name)

    def make(env):
        from chain_compare import compare_track
        from test_gpu_track import Chain
        tracker = env.HS.FrameTracker(env.extractor(tag="track"))
        c, ref = expected()

        @asserted
        def f():
            ch = Chain(tracker, c)
            ch.frame()
            compare_track(ch.results(), c, ref, name, ch.N.LM_DTYPE)
        return f
    return Job("tracking", "TrackFrame %s" % name, expected, make)


def keyframe_job(n, seed=4):
    """FrameTracker.KeyFrameDecision on keyframe_cases.gpu_seeded(n, seed) against ref_keyframe.dense"""
    @functools.lru_cache(maxsize=None)
    def expected():
        import keyframe_cases as KC
        import ref_keyframe as RKF
        c = KC.gpu_seeded(n, seed)
        return c, RKF.dense(c)

    def make(env):
        import ref_keyframe as RKF
        from hyslam_amd import _native as N
        tracker = env.HS.FrameTracker(env.extractor(tag="track"))
        c, want = expected()
        m = min(want["result"]["n_new"], c["new_cap"])

        @asserted
        def f():
            r = tracker.KeyFrameDecision(c["frame"], c["depth"], c["Tcw"], c["T"], c["K"], *c["state"], c["ref_slot"], track_result=c["track"],
                                         params=N.KeyFrameParams(**c["prm"]), new_cap=c["new_cap"])
            assert {k: r[k] for k in RKF.RESULT_KEYS} == want["result"], "result"
            for k in ("kp_lm", "kp_outl", "kp_lm_obs", "lm_index", "offsets"):
                assert np.array_equal(r[k], want[k]), k
            assert r["n_matches"] == want["n_matches"], "n_matches"
            assert np.array_equal(r["new_view"], want["new_view"][:m]), "new_view"
            for k in ("new_pos", "entries", "obs", "desc"):
                assert np.asarray(r[k]).tobytes() == np.asarray(want[k][:m]).tobytes(), k
        return f
    return Job("tracking", "KeyFrameDecision gpu_seeded(%d, %d)" % (n, seed), expected, make)


def projection_host_job():
    """FeatureMatcher.SearchByProjection by host pointers on a 320 x 240, 300-feature projection_scene against the oracle"""
    @functools.lru_cache(maxsize=None)
    def expected():
        import oracle
        import scenes
        sc = scenes.projection_scene(35, 320, 240, nfeat=300, copies=3, fx=260.0)
        Fo, keep = oracle.make_frame_view(oracle.FrameView, **sc["frame_args"])
        want = oracle.search_by_projection(Fo, sc["lms"], oracle.ProjParams(5.0, 100.0, 0.8, 0.5, 1.5, 1, 1, 0))
        assert want[2] > 30
        return sc, want

    def make(env):
        import oracle
        from hyslam_amd import _native as N
        sc, (oi, od, on) = expected()
        m = env.HS.FeatureMatcher(env.HS.FeatureMatcherSettings(nnratio=0.8), env.extractor(tag="match"))
        Fg, keep = oracle.make_frame_view(N.FrameView, **sc["frame_args"])

        @asserted
        def f():
            gi, gd, gn = m.SearchByProjection(Fg, sc["lms"], 5.0)
            assert np.array_equal(gi, oi) and np.array_equal(gd, od) and gn == on, "SearchByProjection"
        f.keep = keep
        return f
    return Job("tracking", "SearchByProjection host pointers 320x240", expected, make)


# ---------------------------------------------------------------- method jobs: mapping
def fuse_job():
    """FeatureMatcher.Fuse as tests/test_gpu_matchers.py::test_fuse compares it, on a 320 x 240 scene"""
    @functools.lru_cache(maxsize=None)
    def expected():
        import oracle
        import scenes
        sc = scenes.projection_scene(39, 320, 240, nfeat=300, copies=4, fx=260.0)
        lms = sc["lms"].copy()
        lms["normal"][::5] *= -1
        lms["skip"][::11] = 1
        Fo, keep = oracle.make_frame_view(oracle.FrameView, **sc["frame_args"])
        pp = oracle.ProjParams(3.0, 50.0, 1.0, 0.5, 1.5, use_distance=1, use_stereo=0, check_rotation=0, use_prev_matched=0,
                               use_viewing_angle=1, max_view_angle=1.047, use_reprojection=1, reproj_threshold=5.99, sigma_ref=1.0, first_wins=1)
        want = oracle.search_by_projection(Fo, lms, pp)
        assert want[2] > 30
        return sc, lms, want

    def make(env):
        import oracle
        from hyslam_amd import _native as N
        sc, lms, (oi, od, on) = expected()
        m = env.HS.FeatureMatcher(env.HS.FeatureMatcherSettings(nnratio=0.8), env.extractor(tag="match"))
        Fg, keep = oracle.make_frame_view(N.FrameView, **sc["frame_args"])

        @asserted
        def f():
            gi, gd, gn = m.Fuse(Fg, lms, 3.0, 5.99)
            assert np.array_equal(gi, oi) and np.array_equal(gd, od) and gn == on, "Fuse"
        f.keep = keep
        return f
    return Job("mapping", "Fuse 320x240", expected, make)


def triangulation_job():
    """FeatureMatcher.SearchForTriangulation on the two views of the 320 x 240 pair (the reference's features), as test_search_for_triangulation_core"""
    @functools.lru_cache(maxsize=None)
    def expected():
        import extract_cases as X
        import oracle
        import scenes
        k1, d1, k2, d2 = X.stereo_reference(0)[:4]
        F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
        rng = np.random.default_rng(8)
        fv1, fv2 = scenes.synthetic_featvec(d1, 7, 13), scenes.synthetic_featvec(d2, 7, 13)
        keep1, keep2 = (rng.random(len(k1)) < 0.85).astype(np.uint8), (rng.random(len(k2)) < 0.85).astype(np.uint8)
        want = oracle.search_by_bow(k1, d1, fv1, k2, d2, fv2, keep1, 90.0, 1.0, True, keep2=keep2, F12=F12)
        assert want[1] > 5
        return (k1, d1, fv1, k2, d2, fv2, F12, keep1, keep2), want

    def make(env):
        args, (om, on) = expected()
        m = env.HS.FeatureMatcher(env.HS.FeatureMatcherSettings(nnratio=0.8, TH_LOW=90.0), env.extractor(tag="match"))

        @asserted
        def f():
            gm, gn = m.SearchForTriangulation(*args)
            assert gn == on and np.array_equal(gm, om), "SearchForTriangulation"
        return f
    return Job("mapping", "SearchForTriangulation 320x240", expected, make)


def landmark_entries_job():
    """FeatureMatcher.UpdateLandmarkEntries on a random_batch of 300 landmarks, one of them with 65 observations (above one wavefront), against
    ref_landmark_entry.update_entries_fast"""
    @functools.lru_cache(maxsize=None)
    def expected():
        import ref_landmark_entry as R
        from landmark_entry_cases import random_batch
        ent, off, ob, descs = random_batch(7, 300, n_max=40, big=[(11, 65), (200, 64)])
        return (ent, off, ob, descs), R.update_entries_fast(ent, off, ob, descs)

    def make(env):
        import ref_landmark_entry as R
        (ent, off, ob, descs), want = expected()
        m = env.HS.FeatureMatcher(extractor=env.extractor(tag="match"))

        @asserted
        def f():
            got = m.UpdateLandmarkEntries(ent, obs_offsets=off, obs=ob, descriptors=descs)
            for k in ("normal", "min_dist", "max_dist", "mean_dist", "size", "best", "median", "flags"):
                assert R.same(got[k], want[k]), k
        return f
    return Job("mapping", "UpdateLandmarkEntries 300 landmarks, one of 65 observations", expected, make)


def refkf_job(name="two_take_one_view"):
    """FrameTracker.SearchByBoWKeyFrame, then AssociateLandMarks on the case's entry state, as tests/test_gpu_refkf.py compares the pair with
    ref_refkf on a directed case of tests/refkf_cases.py"""
    @functools.lru_cache(maxsize=None)
    def expected():
        import ref_refkf as RR
        import ref_track as R
        import refkf_cases as RC
        c, _, (_, rk, _) = RC.directed(name)
        fr, rp = c["frame"], c["rp"]
        bow, internal, want_n = RR.search_by_bow_kf(c["K"], c["kf_slot"], c["kf_cap"], c["T"]["lm_bad"], fr["kps"], fr["desc"], rk["bow_word"], rk["bow_weight"],
                                                    rk["bow_node"], rp.th_low, rp.nnratio)
        want = RR.associate_landmarks(R.MapMatches.from_dense(*c["state0"]), bow).dense(len(fr["kps"]))
        return c, rk, bow, want_n, want

    def make(env):
        c, rk, bow, want_n, want = expected()
        fr, rp, s0 = c["frame"], c["rp"], c["state0"]
        tracker = env.HS.FrameTracker(env.extractor(tag="track"))
        node = np.where(rk["bow_weight"] > 0, rk["bow_node"], -1).astype(np.int32)

        @asserted
        def f():
            matches, match_kf, nm = tracker.SearchByBoWKeyFrame(c["K"], c["kf_slot"], c["T"], fr["kps"], fr["desc"], node, rp.th_low, rp.nnratio, c["kf_cap"])
            assert matches == bow and nm == want_n and np.array_equal(match_kf, rk["match_kf"]), "SearchByBoWKeyFrame"
            got = tracker.AssociateLandMarks(s0[0], s0[1], s0[2], matches, len(c["lms"]))
            for g, w, what in zip(got, want, ("kp_lm", "kp_outl", "n_matches")):
                assert np.array_equal(g, w), what
        return f
    return Job("tracking", "SearchByBoWKeyFrame + AssociateLandMarks %s" % name, expected, make)


# ---------------------------------------------------------------- method jobs: loop closing
PLACE_SCENE = (41, 64, 1000)       # seed, key frames, words


def place_job():
    """PlaceRecognizer on a 64-key-frame random_scene: a recogniser of the call's own is filled (add), a tenth erased, and both kinds of query are
    compared with ref_place as tests/test_gpu_place.py compares them; then it is closed.  add and erase wait for the whole device underneath."""
    @functools.lru_cache(maxsize=None)
    def expected():
        import ref_place as R
        from place_cases import random_scene, ref_query, scene_ref
        seed, n_kf, n_words = PLACE_SCENE
        sc = random_scene(seed, n_kf, n_words, (5, 60), n_queries=4, erase=0.1)
        assert sc["erased"] and {q["mode"] for q in sc["queries"]} == {"reloc", "loop"}
        ref = scene_ref(R, sc)
        return sc, [ref_query(ref, sc, q) for q in sc["queries"]]

    def make(env):
        from test_gpu_place import assert_query, fill, gpu_query
        sc, want = expected()
        ex = env.extractor(tag="place")

        @asserted
        def f():
            rec = fill(env.HS, ex, sc["n_words"], sc["entries"], sc["erased"])
            try:
                assert rec.size() == (PLACE_SCENE[1] - len(sc["erased"]), PLACE_SCENE[1]), "size"
                for i, (q, (want_keys, det)) in enumerate(zip(sc["queries"], want)):
                    keys, got = gpu_query(rec, q, sc["neigh"])
                    assert_query(rec, keys, got, want_keys, det, (i, q["mode"]))
            finally:
                rec.close()
        return f
    return Job("loop", "PlaceRecognizer add / erase / queries 64 key frames", expected, make)


def sim3_job():
    """SearchByProjectionSim3 and SearchBySim3 on one case each of scenes.area_edge_cases, against the oracle"""
    @functools.lru_cache(maxsize=None)
    def expected():
        import oracle
        import scenes
        c = next(x for x in scenes.area_edge_cases(200) if x["kind"] == "mixed")
        s = c["sim3"]
        Fo, keep = oracle.make_frame_view(oracle.FrameView, **c["fa"])
        F2o, keep2 = oracle.make_frame_view(oracle.FrameView, **s["fb"])
        proj = oracle.search_by_projection_sim3(Fo, c["Scw"], c["lms"], c["th"], c["th_low"], c["kp_matched"])
        pair = oracle.search_by_sim3(Fo, s["lms1"], F2o, s["lms2"], s["s12"], s["R12"], s["t12"], s["th"], s["th_high"])
        return c, proj, pair

    def make(env):
        import oracle
        from hyslam_amd import _native as N
        from test_gpu_area_edges import gpu_sim3, gpu_sim3_projection
        c, (oi, ot, on), (om, opn) = expected()
        m = env.HS.FeatureMatcher(env.HS.FeatureMatcherSettings(nnratio=0.8), env.extractor(tag="match"))
        Fg, keep = oracle.make_frame_view(N.FrameView, **c["fa"])
        F2g, keep2 = oracle.make_frame_view(N.FrameView, **c["sim3"]["fb"])

        @asserted
        def f():
            gi, gt, gn = gpu_sim3_projection(m, Fg, c)
            assert np.array_equal(gi, oi) and np.array_equal(gt, ot) and gn == on, "SearchByProjectionSim3"
            gm, gn = gpu_sim3(m, Fg, F2g, c["sim3"])
            assert np.array_equal(gm, om) and gn == opn, "SearchBySim3"
        f.keep = (keep, keep2)
        return f
    return Job("loop", "SearchByProjectionSim3 and SearchBySim3, area edge case", expected, make)


def bow_job():
    """hs_search_by_bow_ex on the list_sizes case of scenes.bow_edge_cases(1), against the oracle"""
    @functools.lru_cache(maxsize=None)
    def expected():
        import oracle
        import scenes
        c = next(x for x in scenes.bow_edge_cases(1) if x["kind"] == "list_sizes")
        want = oracle.search_by_bow(c["k1"], c["d1"], c["fv1"], c["k2"], c["d2"], c["fv2"], c["keep1"], c["score_threshold"], c["ratio"], c["check_rotation"],
                                    keep2=c["keep2"], F12=c["F12"], size_ref=c["size_ref"], sigma_ref=c["sigma_ref"])
        return c, want

    def make(env):
        from test_gpu_bow_edges import native_bow
        c, (om, on) = expected()
        m = env.HS.FeatureMatcher(env.HS.FeatureMatcherSettings(nnratio=0.8), env.extractor(tag="match"))

        @asserted
        def f():
            gm, gn = native_bow(m, c, "ex")
            assert np.array_equal(gm, om) and gn == on, "SearchByBoW"
        return f
    return Job("loop", "SearchByBoW list_sizes", expected, make)


# ---------------------------------------------------------------- host-pointer twins of the case jobs, and the second pose problem
def host_twin(role, name, source, call):
    """the host-pointer form of the entry point a case job runs by device pointers, through the Python mirror: the same real inputs (taken from the
    Case `source()` builds), staged through the worker's handle (its scratch arena and pinned buffers), the same expected bytes.  call(env, case) -> g;
    g() -> {output: array}"""
    def make(env):
        case = job.expected()
        g = call(env, case)

        @asserted
        def f():
            got = {k: _raw(v) for k, v in g().items()}
            return case_mismatch(case, {k: got[k] for k in case.expect})
        return f
    job = Job(role, name, source, make)
    return job


def _real(case, *keys):
    return [case.inputs[k][0] for k in keys]


def _table(case):
    S = _S()
    return {k: case.inputs["T." + k][0] for k in S.TABLE_KEYS}


def _matcher(env):
    return env.HS.FeatureMatcher(extractor=env.extractor(tag="match"))


def host_twins():
    S = _S

    def descriptors(env, c):
        m, (off, desc) = _matcher(env), _real(c, "offsets", "desc")
        return lambda: dict(zip(("best", "median"), m.ComputeDistinctiveDescriptors(offsets=off, desc=desc)))

    def votes(env, c):
        m, T, a = _matcher(env), _table(c), c.args
        qo, ql, sid = _real(c, "q_offsets", "q_lm", "q_self_id")
        return lambda: m.KeyFrameVotes(T, q_offsets=qo, q_lm=ql, self_id=sid, count_bad_kf=bool(a["count_bad_kf"]), th=a["th"], cap=a["cap"])

    def redundancy(env, c):
        m, T, a = _matcher(env), _table(c), c.args
        slot, thd, co, il, io, idp = _real(c, "cand_slot", "cand_th_depth", "cand_offsets", "item_lm", "item_octave", "item_depth")
        return lambda: m.KeyFrameRedundancy(T, slot, thd, cand_offsets=co, item_lm=il, item_octave=io, item_depth=idp, is_mono=bool(a["is_mono"]), th_obs=a["th_obs"],
                                            frac_redundant=a["frac"])

    def local_keyframes(env, c):
        m, a = _matcher(env), c.args
        w, bad, neigh, parent = _real(c, "weights", "kf_bad", "neigh", "parent")

        def g():
            local, n_local = m.LocalKeyFrames(w, bad, np.asarray(neigh).reshape(a["n_kf"], a["neigh_cap"]), parent, a["n_max"], a["n_neighbor"])
            return dict(local=local, n_local=np.array([n_local], np.int32))
        return g

    def local_points(env, c):
        m, T, a = _matcher(env), _table(c), c.args
        local, flm = _real(c, "local", "frame_lm")

        def g():
            rem, sel, n_sel = m.LocalPoints(T, local, flm, a["cap"])
            return dict(frame_remove=rem, sel=sel, n_sel=np.array([n_sel], np.int32))
        return g

    def transform(env, c):
        import scenes
        from hyslam_amd import _native as N
        e = S().vocab_tree()
        voc = env.HS.ORBVocabulary(scenes.tree_struct(N.VocabTree, e["tree"]), env.extractor(tag="match"))
        env.keep.append(e)
        desc, n = _real(c, "desc", "n")
        d = np.ascontiguousarray(desc[:int(n[0])])
        return lambda: dict(zip(("word", "weight", "node"), voc.transform(d, S().LEVELSUP)[2]))

    def vector(env, c):
        import scenes
        from hyslam_amd import _native as N
        e = S().vocab_tree()
        voc = env.HS.ORBVocabulary(scenes.tree_struct(N.VocabTree, e["tree"]), env.extractor(tag="match"))
        env.keep.append(e)
        word, weight, n = _real(c, "word", "weight", "n")
        w, wt = np.ascontiguousarray(word[:int(n[0])]), np.ascontiguousarray(weight[:int(n[0])])

        def g():
            ow, ov = voc.bow_vector(w, wt)
            return dict(out_word=ow, out_value=ov, m=np.array([len(ow)], np.int32))
        return g

    return [
        host_twin("mapping", "ComputeDistinctiveDescriptors, 65 / 129 / 300 observations (host pointers)", lambda: S().landmark_case("large"), descriptors),
        host_twin("mapping", "KeyFrameVotes 64 key frames (host pointers)", lambda: S().kf_votes_case("lds"), votes),
        host_twin("mapping", "KeyFrameRedundancy (host pointers)", lambda: S().kf_redundancy_case(), redundancy),
        host_twin("mapping", "LocalKeyFrames 129 (host pointers)", lambda: S().local_keyframes_case(), local_keyframes),
        host_twin("mapping", "LocalPoints 3 blocks + 1 (host pointers)", lambda: S().local_points_case(), local_points),
        host_twin("loop", "ORBVocabulary.transform 893 descriptors (host pointers)", lambda: S().bow_transform_case(900, (893, 860)), transform),
        host_twin("loop", "ORBVocabulary.bow_vector 4990 entries (host pointers)", lambda: S().bow_vector_case(5000, (4990, 4500)), vector),
    ]


POSE_CASES = ("mixed_out30", "n257")


def pose_host_job():
    """Optimizer::PoseOptimization by host pointers (hs_pose_optimize), Q = 2: the golden cases mixed_out30 (120 edges, 30 of them outliers) and n257 of
    tests/poseopt_cases.py in one call, each held to its golden record as tests/test_gpu_poseopt.py holds it: the flags and the integers exactly,
    Tcw_d within the file's tau, Tcw the float of Tcw_d and within one ulp of the reference's"""
    @functools.lru_cache(maxsize=None)
    def expected():
        import poseopt_cases as P
        g = P.load_golden()
        items = [(g[n + ".T"], g[n + ".cam"], g[n + ".edges"]) for n in POSE_CASES]
        refs = [{k: g[n + "." + k] for k in P.REF_KEYS} for n in POSE_CASES]
        assert int(np.asarray(refs[0]["outlier"]).sum()) > 0 and len(items[0][2]) != len(items[1][2])
        return items, refs, float(g["tau"])

    def make(env):
        import ctypes as C
        from hyslam_amd import _native as N
        items, refs, tau = expected()
        ex = env.extractor(tag="match")
        prob = np.zeros(len(items), N.POSE_PROBLEM_DTYPE)
        for q, (T, cam, _) in enumerate(items):
            prob["Tcw"][q] = np.asarray(T, np.float32).reshape(16)
            for k, v in zip(("fx", "fy", "cx", "cy", "bf"), cam):
                prob[k][q] = v
        off = np.zeros(len(items) + 1, np.int64)
        off[1:] = np.cumsum([len(e) for _, _, e in items])
        edges = np.concatenate([np.ascontiguousarray(e, N.POSE_EDGE_DTYPE) for _, _, e in items])
        p = lambda a: a.ctypes.data_as(C.c_void_p)

        @asserted
        def f():
            outlier = np.full(len(edges), FILL, np.uint8)
            res = np.zeros(len(items), N.POSE_RESULT_DTYPE)
            N.check(ex._h, ex._lib.hs_pose_optimize(ex._h, len(items), p(prob), p(off), p(edges), p(outlier), p(res)))
            for q, (name, ref) in enumerate(zip(POSE_CASES, refs)):
                r = res[q]
                assert np.array_equal(outlier[off[q]:off[q + 1]], ref["outlier"]), "%s: flags" % name
                assert [int(r[k]) for k in ("n_good", "n_edges", "rounds", "status")] == [int(ref[k]) for k in ("n_good", "n_edges", "rounds", "status")], "%s: counts" % name
                assert float(np.abs(r["Tcw_d"].reshape(4, 4) - ref["Tcw_d"]).max()) <= tau, "%s: Tcw_d beyond tau" % name
                assert r["Tcw"].tobytes() == r["Tcw_d"].astype(np.float32).tobytes(), "%s: Tcw is not the float of Tcw_d" % name
                assert np.abs(r["Tcw"].view(np.int32).astype(np.int64) - np.asarray(ref["Tcw"], np.float32).reshape(16).view(np.int32).astype(np.int64)).max() <= 1, "%s: Tcw" % name
        return f
    return Job("tracking", "PoseOptimization mixed_out30 + n257, Q = 2 (host pointers)", expected, make)


# ---------------------------------------------------------------- the table
@functools.lru_cache(maxsize=None)
def jobs():
    S = _S
    J = [
        # image processing: the two extractor threads and the front end
        extract_job("geom_273x225"), extract_job("periodic_ties"), extract_batch_job(), ticket_job(), publish_job(),
        extract_device_job(), stereo_frontend_device_job(),
        case_job("images", "preprocess_device 333x201x3", lambda: S().preprocess_case()),
        case_job("images", "stereo_match_batch_device 3 pairs", lambda: S().stereo_match_case()),
        # tracking
        track_frame_job("narrow"), track_frame_job("wide"), track_frame_job("both_fail"), keyframe_job(65), keyframe_job(1025), projection_host_job(), refkf_job(),
        case_job("tracking", "search_by_projection_device local map", lambda: S().projection_case(False)),
        case_job("tracking", "search_by_projection_posed_device", lambda: S().projection_case(True)),
        case_job("tracking", "local_map_search_device 640x480", lambda: S().local_map_search_case()),
        case_job("tracking", "pose_edges_device 640x480", lambda: S().pose_edges_case()),
        case_job("tracking", "pose_optimize_device n257", lambda: S().pose_optimize_case()),
        # mapping
        case_job("mapping", "landmark_best_descriptors_device, none above 64", lambda: S().landmark_case("small")),
        case_job("mapping", "landmark_best_descriptors_device, 65 / 129 / 300 observations", lambda: S().landmark_case("large")),
        case_job("mapping", "kf_votes_device 64 key frames (LDS counters)", lambda: S().kf_votes_case("lds")),
        case_job("mapping", "kf_votes_device above the LDS slots (global counters)", lambda: S().kf_votes_case("global")),
        case_job("mapping", "kf_redundancy_device", lambda: S().kf_redundancy_case()),
        case_job("mapping", "local_keyframes_device 129", lambda: S().local_keyframes_case()),
        case_job("mapping", "local_points_device 3 blocks + 1", lambda: S().local_points_case()),
        case_job("mapping", "landmark_gather_device 37 of 64", lambda: S().landmark_gather_case()),
        fuse_job(), triangulation_job(), landmark_entries_job(),
        # loop closing
        bow_transform_job(900, (893, 860)), bow_transform_job(200, (200, 150)),
        case_job("loop", "bow_vector_device n_max 5000 (raises the LDS limit)", lambda: S().bow_vector_case(5000, (4990, 4500))),
        case_job("loop", "bow_vector_device n_max 300", lambda: S().bow_vector_case(300, (300, 280))),
        case_job("loop", "hamming_knn2_device 321x517", lambda: S().knn2_case()),
        place_job(), sim3_job(), bow_job(),
        pose_host_job(),
    ] + host_twins()
    assert len({j.name for j in J}) == len(J)
    return J


def by_role(role):
    return [j for j in jobs() if j.role == role]


def worker(job_list):
    """-> setup() for concurrent_harness.run: an Env of the worker's own, every job of the list bound to it"""
    def setup():
        env = Env()
        bound = [(j.name, j.make(env)) for j in job_list]
        setup.env = env
        return bound
    return setup
