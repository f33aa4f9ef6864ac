"""CPU: pins the restatement of MapPointDBEntry::_computeDistinctiveDescriptor_ (tests/ref_landmark.py) that the GPU landmark tests compare against,
on hand-built landmarks whose answers are derived in tests/landmark_cases.py, and against a second formulation (statistics.median_low)."""
import statistics

import numpy as np
import pytest

from landmark_cases import KNOWN, on_line, prefix
from ref_landmark import distinctive_descriptor, distinctive_descriptors, distinctive_descriptors_fast, orb_distance


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(name):
    d, best, median = KNOWN[name]
    assert distinctive_descriptor(d) == (best, median)
    b, m = distinctive_descriptors_fast([d])
    assert (int(b[0]), int(m[0])) == (best, median)


def test_empty_landmark_is_left_alone():
    assert distinctive_descriptor(np.zeros((0, 32), np.uint8)) == (-1, -1)
    b, m = distinctive_descriptors([np.zeros((0, 32), np.uint8), on_line([3])])
    assert b.tolist() == [-1, 0] and m.tolist() == [-1, 0]


def test_distance_is_hamming():
    assert orb_distance(prefix(0), prefix(256)) == 256 and orb_distance(prefix(5), prefix(12)) == 7
    a = np.arange(32, dtype=np.uint8)
    assert orb_distance(a, a) == 0 and orb_distance(a, a ^ np.uint8(1)) == 32


def _mutated(descs, index, strict=True):
    """the reference with a different median index or `<=`: the known answers must tell these apart"""
    d = np.asarray(descs, np.uint8).reshape(-1, 32)
    N = len(d)
    med = [sorted(orb_distance(d[i], d[j]) for j in range(N))[index(N)] for i in range(N)]
    best, bm = 0, float("inf")
    for i, v in enumerate(med):
        if (v < bm) if strict else (v <= bm):
            best, bm = i, v
    return best, bm


def test_known_answers_reject_off_by_one_median_index_and_non_strict_compare():
    d, best, median = KNOWN["n4_lower_median"]
    assert _mutated(d, lambda N: N // 2) != (best, median)
    assert _mutated(d, lambda N: (N - 1) // 2, strict=False) != (best, median)
    d, best, median = KNOWN["n6_index_and_strict"]
    for idx in (lambda N: N // 2, lambda N: (N - 1) // 2 - 1):
        assert _mutated(d, idx)[0] != best
    assert _mutated(d, lambda N: (N - 1) // 2, strict=False)[0] != best
    d, best, median = KNOWN["mean_vs_median"]
    sums = [sum(orb_distance(d[i], d[j]) for j in range(len(d))) for i in range(len(d))]
    assert int(np.argmin(sums)) != best


def test_restatement_agrees_with_median_low_on_random_landmarks():
    rng = np.random.default_rng(5)
    lms = []
    for _ in range(300):
        n = int(rng.integers(0, 24))
        base = rng.integers(0, 256, (3, 32), dtype=np.uint8)             # clustered: few centres, a few flipped bits -> many ties
        d = base[rng.integers(0, 3, n)].copy()
        flips = rng.integers(0, 256, (n, 2))
        for k in range(n):
            for f in flips[k][: int(rng.integers(0, 3))]:
                d[k, f // 8] ^= np.uint8(1 << (f % 8))
        lms.append(d)
    b, m = distinctive_descriptors(lms)
    bf, mf = distinctive_descriptors_fast(lms)
    assert np.array_equal(b, bf) and np.array_equal(m, mf)
    for d, bi, mi in zip(lms, b, m):
        if len(d) == 0:
            continue
        meds = [statistics.median_low([orb_distance(d[i], d[j]) for j in range(len(d))]) for i in range(len(d))]
        assert (bi, mi) == (meds.index(min(meds)), min(meds))
