"""GPU: the host-pointer entry points share one grow-only scratch arena per handle, laid out afresh by every call (HsStage, hs_internal.h).
One handle makes hs_search_by_projection, hs_search_by_bow_ex and hs_landmark_update_entries in sequence, three times: at 40 keypoints with
25 landmarks (the arena's first allocation), at 600 with 2000 (every call regrows it) and at 1 with 1 (every call reuses a far larger arena).
Each result is bit-exact against the reference the entry point's own tests use: the oracle for the two matchers (tests/test_gpu_matchers.py),
the numpy restatement for the landmark entries (tests/test_gpu_landmark_entries.py)."""
import numpy as np
import pytest

import oracle
import ref_landmark_entry as R
import scenes
import hyslam_amd as HS
from hyslam_amd import _native as N
from landmark_entry_cases import random_batch

pytestmark = pytest.mark.gpu

SIZES = ((40, 25), (600, 2000), (1, 1))           # (keypoints, landmarks): first allocation, regrow, reuse
PP = oracle.ProjParams(5.0, 100.0, 0.8, 0.5, 1.5, 1, 1, 0)      # SearchByProjection(Frame, MapPoints, th = 5), as in test_projection_variants_small


def projection_case(sc, n, L):
    """the scene cut to its first n keypoints and L landmarks, the landmarks that those keypoints can match first"""
    fa = dict(sc["frame_args"])
    for k in ("kps", "desc", "uR", "kp_lm_obs"):
        fa[k] = fa[k][:n].copy()
    lms = sc["lms"].copy()
    lms["assoc_kp"][lms["assoc_kp"] >= n] = -1
    Fo, keep = oracle.make_frame_view(oracle.FrameView, **fa)
    oi, _, _ = oracle.search_by_projection(Fo, lms, PP)
    lms = lms[np.argsort(oi < 0, kind="stable")][:L].copy()
    return fa, lms


def bow_case(sc, n, seed):
    """test_bow_grouped_search's pair of views, of the first n features"""
    rng = np.random.default_rng(seed)
    k1, d1 = sc["kps"][:n].copy(), sc["desc"][:n].copy()
    perm = rng.permutation(n)
    k2, d2 = k1[perm].copy(), d1[perm].copy()
    d2[::2, 7] ^= 0x3C
    k2["angle"] = (k2["angle"] + rng.normal(0, 3, n) + (rng.random(n) < 0.15) * 120) % 360
    keep1 = (rng.random(n) < 0.8).astype(np.uint8)
    return k1, d1, scenes.synthetic_featvec(d1, 61, 11), k2, d2, scenes.synthetic_featvec(d2, 61, 11), keep1


def test_one_handle_first_allocation_regrow_and_reuse(gpu):
    matcher = HS.FeatureMatcher(HS.FeatureMatcherSettings(nnratio=0.8), HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=500)))
    sc = scenes.projection_scene(31, 640, 480, nfeat=1000, copies=3)
    assert len(sc["kps"]) >= 600 and len(sc["lms"]) >= 2000
    for rnd, (n, L) in enumerate(SIZES):
        tag = (n, L)
        # hs_search_by_projection
        fa, lms = projection_case(sc, n, L)
        Fo, keep_o = oracle.make_frame_view(oracle.FrameView, **fa)
        Fg, keep_g = oracle.make_frame_view(N.FrameView, **fa)
        oi, od, on = oracle.search_by_projection(Fo, lms, PP)
        gi, gd, gn = matcher.SearchByProjection(Fg, lms, 5.0)
        assert not matcher.frame_on_device                      # the host-pointer entry point, not hs_search_by_projection_frame
        assert gn == on and np.array_equal(gi, oi) and np.array_equal(gd, od), tag
        assert on > 0 or n == 1, tag
        # hs_search_by_bow_ex
        k1, d1, fv1, k2, d2, fv2, keep1 = bow_case(sc, n, 5 + rnd)
        om, on = oracle.search_by_bow(k1, d1, fv1, k2, d2, fv2, keep1, 50.0, 0.8, True)
        gm, gn = matcher.SearchByBoW(k1, d1, fv1, k2, d2, fv2, keep1, True)
        assert gn == on and np.array_equal(gm, om), tag
        assert on > 0 or n == 1, tag
        # hs_landmark_update_entries
        ent, off, ob, descs = random_batch(40 + rnd, L, n_max=40, big=[(0, 70)])
        got = matcher.UpdateLandmarkEntries(ent, obs_offsets=off, obs=ob, descriptors=descs)
        want = R.update_entries_fast(ent, off, ob, descs)
        for k in ("normal", "min_dist", "max_dist", "mean_dist", "size", "best", "median", "flags"):
            assert R.same(got[k], want[k]), tag + (k,)
