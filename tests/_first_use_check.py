"""The first library calls of a process, made by three threads released together (tests/test_gpu_concurrent_handles.py runs this in a child process):
each thread creates a handle, extracts one 1920 x 1080 frame (the small-batch pyramid plan: the deep chain's LDS limit is raised on first use) and
turns a 5000-entry word list into a BoW vector (k_bow_vector raises its limit on every long call).  The expected values are computed before the library
is loaded: the oracle's extraction, ref_place.bow_vector."""
import ctypes as C
import os
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle
import ref_place
from hyslam_amd.synth import synth_image

W, H, NF, N_WORDS = 1920, 1080, 2000, 5000


def main():
    img = synth_image(77, W, H)
    ok, od = oracle.extract(oracle.default_params(NF), img)
    assert len(ok) > 1000
    rng = np.random.default_rng(3)
    word = rng.integers(0, 3000, N_WORDS).astype(np.int32)        # repeated words: their weights add up
    weight = (rng.random(N_WORDS) + 0.1).astype(np.float32)
    ww, wv = ref_place.bow_vector(word, weight)
    ww, wv = np.array(ww, np.int32), np.array(wv, np.float64)
    gate, bad = threading.Barrier(3), []

    def body(t):
        try:
            gate.wait(60)
            import hyslam_amd as HS                                # the first thing this process asks of the library
            from hyslam_amd import _native as N
            ex = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=NF), device=0)
            gk, gd = ex(img)
            if not (len(gk) == len(ok) and gk.tobytes() == ok.tobytes() and np.array_equal(gd, od)):
                bad.append((t, "extraction differs from the oracle", len(gk), len(ok)))
            ow, ov, m = np.zeros(N_WORDS, np.int32), np.zeros(N_WORDS, np.float64), C.c_int32(-1)
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            N.check(ex._h, ex._lib.hs_bow_vector(ex._h, p(word), p(weight), N_WORDS, p(ow), p(ov), C.byref(m)))
            if not (m.value == len(ww) and np.array_equal(ow[:m.value], ww) and ov[:m.value].tobytes() == wv.tobytes()):
                bad.append((t, "bow vector differs from ref_place", m.value, len(ww)))
            gk2, gd2 = ex(img)                                     # once more, now that every first time is behind
            if gk2.tobytes() != ok.tobytes() or not np.array_equal(gd2, od):
                bad.append((t, "second extraction differs"))
        except BaseException as e:
            bad.append((t, "raised", repr(e)[:300]))

    threads = [threading.Thread(target=body, args=(t,), daemon=True) for t in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    if any(t.is_alive() for t in threads):
        print("FIRST_USE_HUNG")
        os._exit(4)
    if bad:
        print("FIRST_USE_FAILED", bad)
        sys.exit(1)
    print("FIRST_USE_OK: %d keypoints, %d words" % (len(ok), len(ww)))


if __name__ == "__main__":
    main()
