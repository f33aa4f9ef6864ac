"""tests/ref_localmap.py — the restatement the GPU tests of hs_local_keyframes / hs_local_points compare against — pinned without a GPU: the literal
version (a Python set walked as a std::set, each key frame's landmark list) and the array version (from the observation table) agree on generated
cases, and both give the hand-derived answers of tests/localmap_cases.py.  Their agreement on the points is the "matches equal observations"
decision."""
import numpy as np
import pytest

import ref_localmap as R
from localmap_cases import KNOWN_KEYFRAMES, KNOWN_POINTS, POINTS_TABLE, random_keyframes, random_points


def _kf_args(c):
    return c["weights"], c["kf_bad"], c["neigh"], c["parent"], c["n_max"], c["n_neighbor"]


@pytest.mark.parametrize("name", sorted(KNOWN_KEYFRAMES))
def test_known_keyframes(name):
    c = KNOWN_KEYFRAMES[name]
    assert sorted(R.local_keyframes_literal(*_kf_args(c))) == c["local"], name
    local, n_local = R.local_keyframes_fast(*_kf_args(c))
    assert np.nonzero(local)[0].tolist() == c["local"] and n_local == len(c["local"]), name


@pytest.mark.parametrize("name", sorted(KNOWN_POINTS))
def test_known_points(name):
    c = KNOWN_POINTS[name]
    selected, removed = R.local_points_literal(R.key_frame_matches(POINTS_TABLE), POINTS_TABLE["lm_bad"], set(np.nonzero(c["local"])[0].tolist()), c["frame_lm"])
    for got in (R.pack_points(selected, removed, len(c["frame_lm"]), c["cap"]), R.local_points_fast(POINTS_TABLE, c["local"], c["frame_lm"], c["cap"])):
        for k in R.POINT_KEYS:
            assert np.array_equal(got[k], np.asarray(c[k])), (name, k, got[k])


def test_keyframes_literal_and_array_agree():
    grew = ended_by_parent = stopped = 0
    for seed in range(300):
        c = random_keyframes(seed, int(np.random.default_rng(seed).choice([1, 7, 40, 64, 65, 129])))
        want = R.local_keyframes_literal(*_kf_args(c))
        local, n_local = R.local_keyframes_fast(*_kf_args(c))
        assert np.nonzero(local)[0].tolist() == sorted(want) and n_local == len(want), seed
        first = set(np.nonzero((c["weights"] > 0) & (c["kf_bad"] == 0))[0].tolist())
        assert first <= want
        grew += len(want) > len(first)
        ended_by_parent += any(c["parent"][s] >= 0 for s in want)
        stopped += len(first) > 0 and 0 <= c["n_max"] < len(want)
    assert grew > 100 and ended_by_parent > 30 and stopped > 30                          # the generator reaches every way the walk can end


def test_points_literal_and_table_agree():
    for seed in range(200):
        rng = np.random.default_rng(seed)
        n_kf, L = int(rng.choice([1, 5, 30])), int(rng.choice([0, 1, 50, 300]))
        T, local, flm = random_points(seed, n_kf, L, max_obs=8, n_assoc=int(rng.choice([0, 1, 40])))
        selected, removed = R.local_points_literal(R.key_frame_matches(T), T["lm_bad"], set(np.nonzero(local)[0].tolist()), flm)
        for cap in (0, max(len(selected) - 1, 0), L):
            assert R.same(R.pack_points(selected, removed, len(flm), cap), R.local_points_fast(T, local, flm, cap)) is None, (seed, cap)


def test_gather_restatement():
    from hyslam_amd._native import LM_DTYPE
    rng = np.random.default_rng(0)
    lms = np.frombuffer(rng.integers(0, 256, 9 * LM_DTYPE.itemsize, dtype=np.uint8).tobytes(), LM_DTYPE).copy()
    out = R.gather(lms, np.array([7, 2, -1, -1], np.int32), 2, 4)
    assert out[0]["desc"].tobytes() == lms[7]["desc"].tobytes() and out[1]["pos"].tobytes() == lms[2]["pos"].tobytes()
    assert out["assoc_kp"].tolist() == [-1] * 4 and out["skip"].tolist() == [0, 0, 1, 1] and not np.frombuffer(out[2:].tobytes(), np.uint8)[:36].any()
