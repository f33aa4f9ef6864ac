"""CPU: pins the restatement of MapPointDBEntry::_updateEntry_ (tests/ref_landmark_entry.py), which the GPU entry-update tests compare against, to
the hand-derived answers of tests/landmark_entry_cases.py.  Each mutant of one arithmetic step must fail at least one of them, and the vectorised
form must agree with the scalar one bit for bit."""
import math

import numpy as np
import pytest

import ref_landmark_entry as R
from landmark_entry_cases import ENTRY_DTYPE, KNOWN_ENTRIES, random_batch

f32, f64 = np.float32, np.float64


def run(c, ops=R.Ops):
    return R.update_entry(c["pos"], c["ref_Ow"], list(c["obs"]), c["descs"], ops=ops)


def matches(got, expect):
    """every pinned output: None = not set, NaN = a NaN, else bit-exact (the sign of a zero included)"""
    for k, want in expect.items():
        g = got[k]
        if want is None or g is None:
            if (want is None) != (g is None):
                return False
            continue
        if k in ("best", "median", "flags"):
            if int(g) != want:
                return False
            continue
        if not R.same(np.asarray(g, f32), np.asarray(want, f32)):
            return False
    return True


@pytest.mark.parametrize("name", sorted(KNOWN_ENTRIES))
def test_known_answers(name):
    c = KNOWN_ENTRIES[name]
    got = run(c)
    assert matches(got, c["expect"]), (name, got, c["expect"])


def test_known_answers_vectorised():
    names = sorted(KNOWN_ENTRIES)
    cs = [KNOWN_ENTRIES[k] for k in names]
    ent = np.zeros(len(cs), ENTRY_DTYPE)
    ent["pos"] = [c["pos"] for c in cs]
    ent["ref_Ow"] = [c["ref_Ow"] for c in cs]
    off = np.zeros(len(cs) + 1, np.int64)
    np.cumsum([len(c["obs"]) for c in cs], out=off[1:])
    ob = np.concatenate([c["obs"] for c in cs])
    fast = R.update_entries_fast(ent, off, ob, [c["descs"] for c in cs])
    slow = R.update_entries(ent, [list(c["obs"]) for c in cs], [c["descs"] for c in cs])
    for k in slow:
        assert R.same(fast[k], slow[k]), k


def test_pythagoras_is_the_textbook_answer():
    got = run(KNOWN_ENTRIES["pythagoras"])
    assert got["normal"] == [f32(0.6), f32(0.8), f32(0.0)] and (got["min_dist"], got["max_dist"]) == (2.5, 10.0)


def test_signed_zero_of_the_normal():
    z1 = run(KNOWN_ENTRIES["neg_zero_n1"])["normal"][2]
    z2 = run(KNOWN_ENTRIES["neg_zero_n2"])["normal"][2]
    assert not math.copysign(1.0, z1) < 0 and not math.copysign(1.0, z2) < 0
    # without the + 0.0f of convertTo the n = 2 component would be -0
    assert math.copysign(1.0, f32(f32(-2.0 ** -149) * f32(0.5))) < 0


def test_huge_coordinates_stay_finite():
    got = run(KNOWN_ENTRIES["huge"])
    assert np.isfinite(got["max_dist"]) and np.isfinite(got["mean_dist"]) and all(np.isfinite(got["normal"]))
    with np.errstate(over="ignore"):
        assert np.isinf(f32(3e20) * f32(3e20))                            # what a float norm would do


# ---- mutants: one step of Ops replaced each ----
class FloatNorm(R.Ops):
    @staticmethod
    def norm(v):
        s = f32(0.0)
        for x in v:
            s = s + f32(x) * f32(x)
        return f64(np.sqrt(s))


class DoubleAlpha(R.Ops):
    @staticmethod
    def alpha(s):
        return f64(1.0) / s


class FusedScaleAdd(R.Ops):
    @staticmethod
    def scale_add(d, a, acc):
        return f32(f64(d) * f64(a) + f64(acc))


class SizeGreaterEqual(R.Ops):
    @staticmethod
    def positive(s):
        return s >= 0.0


class SizeReturnsEarly(R.Ops):
    size_returns_early = True


class PairwiseSum(R.Ops):
    @staticmethod
    def total(values):
        v = [f32(x) for x in values]
        if len(v) <= 1:
            return v[0] if v else f32(0.0)
        h = len(v) // 2
        return PairwiseSum.total(v[:h]) + PairwiseSum.total(v[h:])


class NoZeroFlip(R.Ops):
    @staticmethod
    def divide(x, n):
        return x if n == 1 else f32(x * f32(f64(1.0) / f64(n)))


@pytest.mark.parametrize("mutant", [FloatNorm, DoubleAlpha, FusedScaleAdd, SizeGreaterEqual, SizeReturnsEarly, PairwiseSum, NoZeroFlip],
                         ids=lambda m: m.__name__)
def test_every_mutant_fails_a_known_answer(mutant):
    with np.errstate(all="ignore"):
        failed = [k for k, c in KNOWN_ENTRIES.items() if not matches(run(c, mutant), c["expect"])]
    assert failed, mutant.__name__


def test_vectorised_restatement_agrees_with_the_scalar_one():
    ent, off, ob, descs = random_batch(11, 400, n_max=20, big=[(3, 70), (200, 130)])
    fast = R.update_entries_fast(ent, off, ob, descs)
    slow = R.update_entries(ent, [list(ob[off[i]:off[i + 1]]) for i in range(len(ent))], descs)
    for k in slow:
        assert R.same(fast[k], slow[k]), (k, np.nonzero(~((fast[k] == slow[k]) | (np.isnan(fast[k]) & np.isnan(slow[k]))))[0][:5])
    # the batch reaches the cases it is meant to: NaN normals and sizes, empty landmarks, finite results at large scales
    assert np.isnan(slow["normal"]).any() and np.isnan(slow["size"]).any() and (np.diff(off) == 0).any()
    assert (np.abs(slow["mean_dist"][np.isfinite(slow["mean_dist"])]) > 1e18).any()
