"""The GPU extractor against tests/ref_extract.py on a directed case, stage by stage (check_case); run as a script under different HS_* environments
by test_gpu_extract_edges.py::test_kernel_variants_in_subprocess on the seam, tie, cell-edge and retry cases.  The expected values come from
ref_extract alone: nothing here loads the oracle."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extract_cases as X
import hyslam_amd as HS


def make_extractor(nfeatures, scale, nlevels, n_cells=30, fast_threshold=20, blur_taps=None):
    st = HS.FeatureExtractorSettings(nFeatures=nfeatures, fScaleFactor=scale, nLevels=nlevels, N_CELLS=n_cells)
    return HS.ORBExtractor(st, blur_taps=blur_taps, fast_threshold=fast_threshold)


def assert_features(name, gk, gd, rk, rd):
    assert len(gk) == len(rk), (name, len(gk), len(rk))
    for f in ("octave", "x", "y", "response", "size", "angle"):
        assert np.array_equal(gk[f], rk[f]), (name, f)
    assert gk.tobytes() == rk.tobytes(), name
    assert np.array_equal(gd, rd), name


def check_case(name, ex=None):
    """product mode first, then debug mode: pyramid bytes, candidate sets, selection in order, keypoints and descriptors"""
    c = X.CASES[name]
    rk, rd, g = X.reference(name)
    ex = ex or make_extractor(**X.settings_of(c))
    gk, gd = ex(c["img"])
    assert_features(name, gk, gd, rk, rd)
    ex.set_debug(True)
    gk, gd = ex(c["img"])
    for l in range(c["nlevels"]):
        assert np.array_equal(ex.debug_level(0, l), g["pyramid"][l]), (name, "pyramid", l)
        gc, rc = ex.debug_candidates(0, l), g["candidates"][l].astype(np.int32)
        assert len(gc) == len(rc), (name, "candidate count", l, len(gc), len(rc))
        if len(gc):
            assert np.array_equal(gc[np.lexsort((gc[:, 0], gc[:, 1]))], rc[np.lexsort((rc[:, 0], rc[:, 1]))]), (name, "candidates", l)
        gs, rs = ex.debug_selected(0, l), g["selected"][l]
        assert len(gs) == len(rs), (name, "selection count", l, len(gs), len(rs))
        assert np.array_equal(gs.astype(np.float32), rs), (name, "selection order", l)
    assert_features(name, gk, gd, rk, rd)
    ex.set_debug(False)
    return ex


def main():
    for name in X.VARIANT_CASES:
        check_case(name)
    # the batch of mixed content under the same environment
    ex = make_extractor(**X.GEOM)
    ks, ds = ex.extract_batch([X.CASES[n]["img"] for n in X.BATCH_273x225])
    for n, gk, gd in zip(X.BATCH_273x225, ks, ds):
        assert_features(n, gk, gd, *X.reference(n)[:2])
    print("EXTRACT_EDGES_OK", {k: v for k, v in os.environ.items() if k.startswith("HS_")})


if __name__ == "__main__":
    main()
