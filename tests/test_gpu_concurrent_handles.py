"""GPU: the threading contract of include/hyslam_amd.h — a handle belongs to one thread at a time, distinct handles are fully
concurrent — held for every subsystem, not the extractor alone.  The jobs and their expected values come from tests/concurrent_jobs.py (the references,
never the device); tests/concurrent_harness.py runs them on worker threads that own their handles, streams and buffers and are released together.

  serial            every job alone on a fresh handle: the inputs and the comparisons are right before any thread starts
  four roles        image processing, tracking, mapping and loop closing at once, one thread each, as the host system runs them
  one role x 4      the same job list on four threads: the same kernels on four handles at once (whatever a launcher shares per process or per device)
  three handles     ONE host thread, three handles, three caller streams, the resident chain enqueued alternately with no host wait in between: overlap on
                    the device that does not hang on how the interpreter schedules threads
  shared objects    the frame cache (below and above its 16 slots), one device vocabulary under three handles, one place database under a lock beside
                    a second one without, each while another worker keeps the device busy
  first use         a fresh child process whose first library calls come from three threads at once

A multi-thread test counts only if at least half of every worker's calls overlapped a call of another worker on the host clock (Result.check); the
shares are printed.  Nothing here breaks the contract on purpose: no handle is shared, hs_records_bow_match_device is left out."""
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import concurrent_harness as CH
import concurrent_jobs as CJ

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 120.0


@pytest.fixture(autouse=True)
def nothing_more_after_a_hang_or_a_device_error():
    """a worker that hung, or a HIP error a test left behind (a fault is sticky), ends the module's run: nothing more is started on that device"""
    yield
    import hipmem
    if _HUNG:
        pytest.exit("workers %s did not finish: nothing more is started on the device" % _HUNG, returncode=3)
    rc = hipmem.hip().hipDeviceSynchronize()
    if rc != 0:
        pytest.exit("hipError %d after this test: nothing more is started on the device" % rc, returncode=3)


_HUNG = []


def run(workers, rounds, tag, keep_going=False):
    t0 = time.time()
    r = CH.run(workers, rounds, limit_s=LIMIT_S, keep_going=keep_going)
    _HUNG.extend(r.hung)
    print("%s: %s (%.2f s with setup)" % (tag, r.report(), time.time() - t0))
    if not r.hung:                                                # every worker's handles, streams and buffers go now, not at some later collection
        for w in workers:
            env = getattr(w[1], "env", None)
            if env is not None:
                w[1].env = None
                env.close()
    r.check()
    return r


# ---------------------------------------------------------------- serial
@pytest.mark.parametrize("role", CJ.ROLES)
def test_every_job_alone_on_a_fresh_handle(gpu, role):
    for job in CJ.by_role(role):
        env = CJ.Env()
        f = job.make(env)
        for k in range(2):                                        # twice: the second call reuses the handle's arena and the refilled outputs
            out = f()
            assert out is None, (job, k, out)
        del f
        env.close()


# ---------------------------------------------------------------- threads
def test_four_roles_at_once(gpu):
    run([(role, CJ.worker(CJ.by_role(role))) for role in CJ.ROLES], rounds=3, tag="four roles", keep_going=True)         # the lists differ in length: everyone runs until the slowest is done


@pytest.mark.parametrize("role", CJ.ROLES)
def test_one_role_on_four_threads(gpu, role):
    run([("%s %d" % (role, i), CJ.worker(CJ.by_role(role))) for i in range(4)], rounds=2, tag="%s x 4" % role, keep_going=True)


# ---------------------------------------------------------------- one host thread, three handles, three caller streams
def test_three_handles_three_streams_no_host_wait(gpu):
    """slots A (300 views), B (33: below one wave) and G (257, mono) of tests/chain_run.py on handles X, Y and Z, each handle with a caller stream and a
    block of its own (tests/test_gpu_chain_run.py's layout: every field with guard bytes behind it), the three in rotated orders.  Frame i of every
    handle is enqueued before frame i + 1 of any: hs_track_frame_device, hs_track_keyframe_device and hs_landmark_update_entries_device, then a
    device-to-device snapshot of the block on the same stream.  No host wait until everything is enqueued; then every frame is compared as the chain
    runs compare it (the reference, the case alone in fresh buffers, every byte outside the frame's extents and every guard byte untouched)."""
    import hipmem
    import hyslam_amd as HS
    import chain_run as CR
    import test_gpu_chain_run as G
    from hyslam_amd import _native as N
    fr = CR.run()
    alone_tracker = HS.FrameTracker(HS.ORBExtractor(device=0))
    for s in "ABG":                                               # the cases alone, on a handle of their own, before anything overlaps
        G.alone(alone_tracker, N, fr[s], s)
    orders = ("ABG", "BGA", "GAB")
    H = []
    for order in orders:
        tracker = HS.FrameTracker(HS.ORBExtractor(device=0))
        frames = [fr[s] for s in order]
        blk = G.chain_block(tracker, N, frames, 0x55, 5)
        H.append(dict(tracker=tracker, frames=frames, blk=blk, inputs=[G.Inputs(N, f) for f in frames], st=hipmem.Stream(non_blocking=True),
                      snaps=[hipmem.DevBuf(blk.total, zero=False) for _ in frames]))
    hipmem.sync()
    for h in H:
        h["before"] = h["blk"].snapshot()
    t0 = time.time()
    for i in range(3):                                            # no host call that waits from here ...
        for h in H:
            G.enqueue(h["tracker"], N, h["blk"], h["inputs"][i], i % 2, h["st"])
            hipmem.copy_async(h["snaps"][i].ptr, h["blk"].buf.ptr, h["blk"].total, h["st"])
    t_enq = time.time() - t0
    for h in H:                                                   # ... to here: one wait
        h["st"].synchronize()
    print("three handles: 9 frames enqueued in %.1f ms, drained %.1f ms later" % (1e3 * t_enq, 1e3 * (time.time() - t0 - t_enq)))
    for order, h in zip(orders, H):
        before = h["before"]
        for i, f in enumerate(h["frames"]):
            after = h["snaps"][i].to_numpy(np.uint8, h["blk"].total)
            G.check_frame(h["tracker"], N, h["blk"], before, after, f, i % 2, h["inputs"][i], ("three handles", order, i, f.slot))
            before = after


# ---------------------------------------------------------------- shared objects
def busy():
    """a worker that keeps the device busy with the mapping jobs until the others are done"""
    return ("busy", CJ.worker([j for j in CJ.by_role("mapping") if "_device" in j.name]), CH.BACKGROUND)


_FRAMES = {}


def cache_frames(count, first_seed=200):
    """`count` distinct 320 x 240 frames: the oracle's extraction, 200 landmarks around its keypoints and the oracle's local-map search over them"""
    import extract_cases as X
    import oracle
    import scenes
    from hyslam_amd.synth import synth_image
    kw, f32 = X.STEREO, np.float32
    out = []
    for seed in range(first_seed, first_seed + count):
        if seed not in _FRAMES:
            img = synth_image(seed, 320, 240)
            k, d = oracle.extract(oracle.default_params(kw["nfeatures"], kw["scale"], kw["nlevels"]), img)
            rng = np.random.default_rng(seed)
            n = len(k)
            assert n > 50
            fa = dict(Rcw=np.eye(3, dtype=f32), tcw=np.zeros(3, f32), fx=260.0, fy=260.0, cx=160.0, cy=120.0, mbf=26.0, sensor=1, bounds=(0.0, 320.0, 0.0, 240.0),
                      kps=k, desc=d, uR=(k["x"] - rng.uniform(1, 20, n)).astype(f32), kp_lm_obs=rng.integers(-1, 3, n).astype(np.int32), size_ref=31.0)
            lms = scenes._area_landmarks(rng, fa, rng.integers(0, n, 200), rng.choice([0, 3, 20], 200))
            Fo, keep = oracle.make_frame_view(oracle.FrameView, **fa)
            _FRAMES[seed] = dict(img=img, fa=fa, lms=lms, want=oracle.search_by_projection(Fo, lms, oracle.ProjParams(5.0, 100.0, 0.8, 0.5, 1.5, 1, 1, 0)))
        out.append(_FRAMES[seed])
    return out


def cache_worker(frames, published, publish=(), search=(), must_hit=False, clear=False):
    """a worker on the frame cache with a handle of its own: `publish` / `search`: indices into `frames`.  A published frame's index goes into
    `published` (under its lock) once its token exists.  A search takes the next of its indices that is published (the first of them by host pointers
    while none is): FeatureMatcher._project finds the token by the keypoints, searches the device copy, and searches by host pointers where the cache
    refuses with HS_ERR_INVALID; any other status raises.  must_hit: the search must have run on the device copy."""
    def setup():
        import oracle
        from hyslam_amd import _native as N
        env = CJ.Env()
        ex = env.extractor(tag="cache", **CJ._stereo_settings())
        m = env.HS.FeatureMatcher(env.HS.FeatureMatcherSettings(nnratio=0.8), ex)
        views = {i: oracle.make_frame_view(N.FrameView, **frames[i]["fa"]) for i in search}
        stats = setup.stats = dict(hits=0, fallbacks=0, early=0, refused_publish=0, clears={})
        turn = [0]

        def pub(i):
            @CJ.asserted
            def f():
                try:
                    (k,), (d,) = ex.extract_batch([frames[i]["img"]], publish=True)
                except N.HsError as e:                             # every slot is being read: the frame is not published, nothing else is wrong
                    assert e.status == N.HS_ERR_CAPACITY, "publish: status %d" % e.status
                    stats["refused_publish"] += 1
                    return None
                assert k.tobytes() == frames[i]["fa"]["kps"].tobytes() and np.array_equal(d, frames[i]["fa"]["desc"]), "extraction"
                assert ex.last_frame_tokens[0] != 0, "no token"
                with published[1]:
                    published[0].add(i)
            return f

        @CJ.asserted
        def find():
            with published[1]:
                ready = [i for i in search if i in published[0]]
            i = ready[turn[0] % len(ready)] if ready else search[0]
            turn[0] += 1
            gi, gd, gn = m.SearchByProjection(views[i][0], frames[i]["lms"], 5.0)
            oi, od, on = frames[i]["want"]
            assert np.array_equal(gi, oi) and np.array_equal(gd, od) and gn == on, "search of frame %d (%s)" % (i, "device copy" if m.frame_on_device else "host pointers")
            stats["hits" if m.frame_on_device else "fallbacks" if ready else "early"] += 1
            assert m.frame_on_device or not (must_hit and ready), "frame %d is published and was not found on the device" % i

        @CJ.asserted
        def wipe():
            st = ex._lib.hs_frame_cache_clear(0)
            stats["clears"][st] = stats["clears"].get(st, 0) + 1
            assert st in (N.HS_OK, N.HS_ERR_INVALID), "hs_frame_cache_clear: status %d" % st
            if st == N.HS_OK:
                with published[1]:
                    published[0].clear()
        setup.env = env
        jobs = [("publish %d" % i, pub(i)) for i in publish] + [("search", find)] * (len(search) and max(len(publish), 4))
        return jobs + ([("clear", wipe)] if clear else [])
    return setup


def test_frame_cache_below_its_slots_every_lookup_hits(gpu):
    """phase 1: one publisher, 8 distinct frames (the cache has 16 slots: nothing is pushed out), each published once and kept; two readers with handles
    of their own.  A lookup of a frame that is published must find it and search the device copy; the result is the host-pointer search's (the
    oracle's) either way"""
    import hyslam_amd as HS
    assert HS.ORBExtractor(device=0)._lib.hs_frame_cache_clear(0) == 0
    frames, published = cache_frames(8), (set(), threading.Lock())
    pub = cache_worker(frames, published, publish=range(8))
    readers = [cache_worker(frames, published, search=list(range(8))[::s], must_hit=True) for s in (1, -1)]
    r = run([("publisher", pub, 1), ("reader 0", readers[0]), ("reader 1", readers[1]), busy()], rounds=4, tag="frame cache, 8 frames")
    print("frame cache, 8 frames:", [w.stats for w in readers])
    assert all(w.stats["hits"] > 0 and w.stats["fallbacks"] == 0 for w in readers)
    assert HS.ORBExtractor(device=0)._lib.hs_frame_cache_clear(0) == 0


def test_frame_cache_above_its_slots_exact_or_refused(gpu):
    """phase 2: two publishers cycle through 10 frames each (20 > 16 slots: the oldest are pushed out while readers hold tokens); every search returns
    the exact result from the device copy, or is refused with HS_ERR_INVALID and is then exact by host pointers — never a third outcome.  The second
    reader also calls hs_frame_cache_clear while the publishers are active: HS_OK or HS_ERR_INVALID, and no wrong result afterwards"""
    frames, published = cache_frames(20), (set(), threading.Lock())
    pubs = [cache_worker(frames, published, publish=range(0, 10)), cache_worker(frames, published, publish=range(10, 20))]
    readers = [cache_worker(frames, published, search=list(range(20))), cache_worker(frames, published, search=list(range(19, -1, -1)), clear=True)]
    run([("publisher 0", pubs[0]), ("publisher 1", pubs[1]), ("reader 0", readers[0], 6), ("reader 1", readers[1], 6)], rounds=3, tag="frame cache, 20 frames", keep_going=True)
    print("frame cache, 20 frames:", [w.stats for w in pubs + readers])
    assert sum(w.stats["hits"] for w in readers) > 0
    import hyslam_amd as HS
    assert HS.ORBExtractor(device=0)._lib.hs_frame_cache_clear(0) == 0


def test_one_device_vocabulary_under_three_handles(gpu):
    """one hs_vocab_upload, then hs_bow_transform_device from three threads, each through a handle and a stream of its own (the header: "may run
    concurrently on one hs_vocab_dev")"""
    import ctypes as C
    import hyslam_amd as HS
    import scenes
    import stream_order_cases as S
    from hyslam_amd import _native as N
    from hyslam_amd import distributed as D
    owner = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=S.NF), device=0)
    e = S.vocab_tree()
    voc = D.DeviceVocabulary(owner, scenes.tree_struct(N.VocabTree, e["tree"]), S.LEVELSUP, keepalive=e["tree"])
    cases = [j.expected() for j in CJ.by_role("loop") if j.name.startswith("bow_transform_device")]
    assert len(cases) == 2

    class Through:                                                # the shared vocabulary through the worker's own handle
        def __init__(self, ex):
            self.ex = ex

        def transform_device(self, d_desc, d_n, n_max, d_word, d_weight, d_node, stream=0):
            ex = self.ex
            N.check(ex._h, ex._lib.hs_bow_transform_device(ex._h, voc._v, C.c_void_p(d_desc), C.c_void_p(d_n) if d_n else None, n_max, C.c_void_p(d_word),
                                                           C.c_void_p(d_weight), C.c_void_p(d_node), C.c_void_p(stream) if stream else None))

    def worker(order):
        def setup():
            env = CJ.Env()
            setup.env = env
            ex = env.extractor(S.NF)
            return [("bow_transform_device %s on the shared vocabulary" % c.name, CJ.bind_case(c, ex, env.stream, voc=Through(ex))) for c in cases[::order]]
        return setup
    run([("transform 0", worker(1)), ("transform 1", worker(-1)), ("transform 2", worker(1)), busy()], rounds=12, tag="one vocabulary, three handles", keep_going=True)
    voc.close()


def test_place_database_under_a_lock_beside_one_without(gpu):
    """one PlaceRecognizer takes adds from one thread and queries from another under a lock (the adaptor's discipline: HipPlaceRecognizer::mutex), while a
    second recogniser is filled, erased from, queried and closed on a third thread without any lock: add and erase wait for the whole device underneath
    everyone else's work.  Every query of the shared one is compared with ref_place at exactly the entries added so far"""
    import hyslam_amd as HS
    import ref_place as R
    from place_cases import random_scene, ref_query
    from test_gpu_place import assert_query, gpu_query
    seed, n_kf, n_words = CJ.PLACE_SCENE
    sc = random_scene(seed + 1, n_kf, n_words, (5, 60), n_queries=4, erase=0.0)
    lock = threading.Lock()
    owner = HS.ORBExtractor(device=0)                             # the recogniser's handle: used under the lock only
    rec, ref = HS.PlaceRecognizer(n_words, owner), R.PlaceRecognizerRef(n_words)
    state = dict(next=0, queries=0)

    def add_one():
        key, w, v = sc["entries"][state["next"]]
        rec.add(key, (w, v))
        ref.add(key, w, v)
        state["next"] += 1
    FIRST, ROUNDS, ADDS = 30, 8, 4                                # the places come twice: from 32 entries on the queries have loops to find
    for _ in range(FIRST):
        add_one()
    assert FIRST + ROUNDS * ADDS <= n_kf

    @CJ.asserted
    def add():
        with lock:
            add_one()

    def query(q):
        @CJ.asserted
        def f():
            with lock:
                known = {e[0] for e in sc["entries"][:state["next"]]}
                neigh = {k: [x for x in v if x in known] for k, v in sc["neigh"].items() if k in known}
                qq = dict(q, connected=[k for k in q["connected"] if k in known])
                keys, got = gpu_query(rec, qq, neigh)
                want_keys, det = ref_query(ref, dict(sc, neigh=neigh), qq)
                assert_query(rec, keys, got, want_keys, det, (state["next"], q["mode"]))
                state["queries"] += 1
        return f
    alone_job = next(j for j in CJ.by_role("loop") if j.name.startswith("PlaceRecognizer"))
    run([("adder", lambda: [("add", add)] * ADDS), ("querier", lambda: [("query %s %d" % (q["mode"], i), query(q)) for i, q in enumerate(sc["queries"])]),
         ("second database", CJ.worker([alone_job])), busy()], rounds=ROUNDS, tag="place databases")
    assert state["next"] == FIRST + ROUNDS * ADDS and state["queries"] == ROUNDS * len(sc["queries"])
    rec.close()


# ---------------------------------------------------------------- first use
def test_first_use_from_three_threads_in_a_fresh_process(gpu):
    """a child process (started, never exec'ed into) whose FIRST library calls are made by three threads released together: handle creation, the first
    launch of every extractor kernel, the per-device LDS-limit raises and the once-per-process reads of the tuning variables all happen on several
    threads at once.  Each thread extracts one 1920 x 1080 frame (batch 1: the small-batch pyramid plan, levels 1-7 in ONE k_resize_chain launch that asks
    for 36 464 B of dynamic LDS — `host_sanitize plan 1920 1080`; no geometry of the parity sweep plans a chain above 64 KiB, but the launcher raises
    the kernel's limit to 120 KiB on the first deep chain of a device whatever the chain asks for, and that first time is what three threads race
    through here) and turns a 5000-entry word list into a BoW vector (n > 4096: k_bow_vector raises its own limit, on every long call).  Everything is
    compared with the oracle / ref_place inside the child."""
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_first_use_check.py")], env=e, capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:], "%.2f s" % (time.time() - t0))
    assert r.returncode == 0 and "FIRST_USE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
