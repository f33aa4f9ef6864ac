"""tests/ref_kfgraph.py — the restatement the GPU tests of hs_kf_votes / hs_kf_redundancy compare against — pinned without a GPU: the literal
(dict and list) version and the vectorised one agree on generated cases, and both give the hand-derived answers of tests/kfgraph_cases.py."""
import numpy as np
import pytest

import ref_kfgraph as R
from kfgraph_cases import (KNOWN_REDUNDANCY, KNOWN_REDUNDANCY_TABLE, KNOWN_VOTES, csr, key_frame_queries, random_candidates, random_table)


@pytest.mark.parametrize("name", sorted(KNOWN_VOTES))
@pytest.mark.parametrize("impl", [R.votes_literal, R.votes_fast])
def test_known_votes(name, impl):
    c = KNOWN_VOTES[name]
    off, q_lm = csr(c["queries"])
    got = impl(c["T"], off, q_lm, np.asarray(c["self_id"], np.int64), c["count_bad_kf"], c["th"], c["cap"])
    for k in R.VOTE_KEYS:
        assert np.array_equal(got[k], np.asarray(c[k])), (name, k, got[k])


@pytest.mark.parametrize("name", sorted(KNOWN_REDUNDANCY))
@pytest.mark.parametrize("impl", [R.redundancy_literal, R.redundancy_fast])
def test_known_redundancy(name, impl):
    c = KNOWN_REDUNDANCY[name]
    off, flat = csr([np.asarray(r, np.float64).reshape(-1, 3) for r in c["items"]], np.float64)
    flat = flat.reshape(-1, 3)
    got = impl(KNOWN_REDUNDANCY_TABLE, c["cand_slot"], c["cand_th_depth"], off, flat[:, 0].astype(np.int32), flat[:, 1].astype(np.int32),
               flat[:, 2].astype(np.float32), c["is_mono"], c["th_obs"], c["frac"])
    for k in R.RED_KEYS:
        assert np.array_equal(got[k], np.asarray(c[k])), (name, k, got[k])


@pytest.mark.parametrize("seed,count_bad_kf,th", [(0, 0, 15), (1, 1, 15), (2, 0, 1), (3, 1, 4)])
def test_votes_literal_and_vectorised_agree(seed, count_bad_kf, th):
    T = random_table(seed, 24, 400, max_obs=12, big=[(3, 24)])
    off, q_lm, ids = key_frame_queries(T)
    rng = np.random.default_rng(seed)
    extra = [rng.integers(0, 400, 150), [], rng.integers(0, 400, 30).repeat(2)]          # frame-shaped, empty, duplicates
    eoff, elm = csr(extra)
    off = np.concatenate([off, off[-1] + eoff[1:]])
    q_lm = np.concatenate([q_lm, elm])
    ids = np.concatenate([ids, [-1, -1, int(T["kf_id"][1])]])
    for cap in (3, 10, 30):
        a = R.votes_literal(T, off, q_lm, ids, count_bad_kf, th, cap)
        b = R.votes_fast(T, off, q_lm, ids, count_bad_kf, th, cap)
        assert R.same(a, b, R.VOTE_KEYS) is None
        assert a["ordered"] == b["ordered"]
    assert a["n_ordered"].max() > 3 and (a["max_slot"] >= 0).any()


@pytest.mark.parametrize("seed,is_mono,th_obs,frac", [(0, 0, 3, 0.9), (1, 1, 3, 0.9), (2, 0, 2, 0.5), (3, 1, 1, 0.25)])
def test_redundancy_literal_and_vectorised_agree(seed, is_mono, th_obs, frac):
    T = random_table(seed, 24, 400, max_obs=12, big=[(3, 24)])
    c = random_candidates(seed, T, [0, 1, 63, 64, 65, 300])
    args = (T, c["cand_slot"], c["cand_th_depth"], c["cand_offsets"], c["item_lm"], c["item_octave"], c["item_depth"], is_mono, th_obs, frac)
    a, b = R.redundancy_literal(*args), R.redundancy_fast(*args)
    assert R.same(a, b, R.RED_KEYS) is None
    assert a["n_redundant"].max() > 0 and a["n_mps"][0] == 0 and not a["cull"][0]
