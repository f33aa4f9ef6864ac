"""CPU: pins tests/ref_place.py (the restatement of src/core/PlaceRecognizer.cpp:43-311, DBoW2's L1 score and the BoW vector) to hand-derived
cases, and shows that each of a handful of deliberate mistakes in it is caught by at least one of them.  tests/test_gpu_place.py then holds the
library to this restatement bit for bit."""
import numpy as np
import pytest

import ref_place as R
from place_cases import BOW_LAST_BIT, KNOWN, SCENES, random_scene, ref_query, run_ref, scene_ref


def check_case(case, mutate=None):
    """-> list of what differs from the hand-derived expectation"""
    out, det, _ = run_ref(R, case, mutate)
    bad = []
    if out != case["expect"]:
        bad.append(("candidates", out, case["expect"]))
    if "words" in case and (det["words"] != case["words"] if not case["words"] else any(det["words"].get(k) != v for k, v in case["words"].items())):
        bad.append(("words", det["words"], case["words"]))
    for name in ("score", "acc"):
        for k, v in case.get(name, {}).items():
            got = det[name].get(k)
            if got is None or np.float32(got).tobytes() != np.float32(v).tobytes():
                bad.append((name, k, got, v))
    for k, v in case.get("best", {}).items():
        if det["best"].get(k, -1) != v:
            bad.append(("best", k, det["best"].get(k, -1), v))
    return bad


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_case(name):
    assert check_case(KNOWN[name]) == []


def test_identical_vectors_score_one_and_disjoint_vectors_nothing():
    v = [(1, 0.25), (2, 0.25), (5, 0.5)]
    assert R.l1_score(v, v) == 1.0
    assert R.l1_score(v, [(3, 0.5), (4, 0.5)]) == 0.0
    # |0.5 - 0.25| - 0.5 - 0.25 = -0.5 on the one shared word
    assert R.l1_score([(1, 0.5), (2, 0.5)], [(2, 0.25), (3, 0.75)]) == 0.25


def test_min_common_words_is_a_float_product_truncated():
    ref = R.PlaceRecognizerRef(1)
    assert [ref._min_common(n) for n in (0, 1, 4, 5, 9, 10, 31, 32)] == [0, 0, 3, 4, 7, 8, 24, 25]
    # 5 242 881 * 0.8f = 4 194 305.4...: the float product rounds to 4 194 305.5 (floats are 0.5 apart there); in double 4 194 304.8
    assert ref._min_common(5242881) == 4194305
    assert R.PlaceRecognizerRef(1, "double_product")._min_common(5242881) == 4194304


def test_bow_vector_sums_in_feature_order():
    c = BOW_LAST_BIT
    assert R.bow_vector(c["word"], np.float32(c["weight"])) == c["expect"]
    assert R.bow_vector(c["word"], np.float32(c["weight"]), order="sorted") == c["sorted_expect"]
    assert R.bow_vector([4, 2], np.float32([0.0, -1.0])) == ([], [])


def test_erase_and_clear():
    case = KNOWN["tombstoned_neighbour"]
    _, _, ref = run_ref(R, case)
    assert 9 not in ref.bow and all(9 not in lst for lst in ref.inverted)
    ref.clear()
    assert ref.detect_reloc(*case["query"], {}) == ([], dict(words={}, score={}, acc={}, best={}))


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_fails_a_case(mutant):
    failed = [name for name in sorted(KNOWN) if check_case(KNOWN[name], mutant)]
    if mutant == "double_product":                         # differs from the float product only from 5 242 881 shared words on: pinned on the helper
        ref = R.PlaceRecognizerRef(1, mutant)
        failed += ["min_common(5242881)"] if ref._min_common(5242881) != 4194305 else []
    assert failed, mutant


def test_seeded_scenes_meet_their_conditions():
    """the conditions tests/test_gpu_place.py relies on, checked with the restatement alone: every branch is taken, and at least half the queries
    return two or more candidates"""
    trace, n_q, n_multi = {}, 0, 0
    for seed, n_kf, n_words, lens, big, n_queries in SCENES:
        if n_kf > 1000:
            n_q += n_queries                                # the large scenes are walked in the GPU test: counted here as if none returned two
            continue
        sc = random_scene(seed, n_kf, n_words, lens, big, n_queries)
        ref = scene_ref(R, sc)
        for q in sc["queries"]:
            out, det = ref_query(ref, sc, q)
            n_q += 1
            n_multi += len(out) >= 2
        for k, v in ref.trace.items():
            trace[k] = trace.get(k, 0) + v
    for branch in ("replace", "dedupe", "excluded", "d9", "tombstone"):
        assert trace.get(branch, 0) > 0, (branch, trace)
    assert 2 * n_multi >= n_q, (n_multi, n_q)
