"""CPU: what keeps the map-side sweep (tools/fuzz_map.py, tests/test_gpu_fuzz_map.py) honest — generators and references only, no device.

  * every family's committed slice (seed, case count) reaches every tag of its list; the tags come from the reference's result alone
  * concatenating cases with disjoint view and landmark ranges is sound: the module's sequential loops on the concatenated state of a strided
    sample of the 3 x 3 spaces equal seq_batch case by case, and the slip `minw[u] > k` in a closed form is caught through the concatenation
  * a planted mismatch — one element of one output array of the reference's result changed, once for every output array — is reported by name
  * the generators called with their default parameters still produce the bytes they produced before they grew parameters"""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_map as FM                           # noqa: E402
import keyframe_cases as KF                     # noqa: E402
import kfgraph_cases as KC                      # noqa: E402
import landmark_entry_cases as LE               # noqa: E402
import localmap_cases as LM                     # noqa: E402
import place_cases as PL                        # noqa: E402
import ref_refkf as RR                          # noqa: E402
import ref_track as R                           # noqa: E402
import refkf_cases as RC                        # noqa: E402
import track_cases as TC                        # noqa: E402


@pytest.mark.parametrize("name", list(FM.FAMILIES))
def test_slice_reaches_every_tag(name):
    fam = FM.FAMILIES[name]
    seen = fam.reach()
    assert set(seen) == set(fam.tags), (sorted(set(fam.tags) - set(seen)), sorted(set(seen) - set(fam.tags)))


# ---------------------------------------------------------------- concatenation
def _sequential(which):
    def run(s):
        n = len(s["kp_lm"])
        f = R.replay_sequential if which == "lm" else RR.replay_views_sequential
        return f(R.MapMatches.from_dense(s["kp_lm"], s["kp_outl"], s["n_matches"]), s["op_view"], s["op_lm"], n, s["L"]).dense(n)
    return run


@pytest.mark.parametrize("which", ["lm", "vw"])
def test_concatenation_is_sound(which):
    """every 37th case of the 3 x 3 space as ONE state of ~9 000 (lm) / ~4 800 (vw) views, ops in shuffled array order, through the literal loop"""
    count, msg = FM.exhaustive_check(which, 3, 3, _sequential(which), seed=5, stride=37)
    assert msg is None, msg
    assert count == {"lm": -(-110592 // 37), "vw": -(-58752 // 37)}[which]


def test_a_slip_in_the_closed_form_shows_through_the_concatenation():
    """`minw[u] > k` for `>=` in the landmark-order closed form, run on the concatenated 3 x 3 space: found, with the case's own state in the message"""
    strict = lambda s: R.replay_closed_form(s["kp_lm"], s["kp_outl"], s["n_matches"], s["op_view"], s["op_lm"], s["L"], minw_strict=True)
    count, msg = FM.exhaustive_check("lm", 3, 3, strict, seed=5, stride=7)
    assert msg is not None and "exhaustive 3 x 3" in msg and "state [" in msg
    right = lambda s: R.replay_closed_form(s["kp_lm"], s["kp_outl"], s["n_matches"], s["op_view"], s["op_lm"], s["L"])
    assert FM.exhaustive_check("lm", 3, 3, right, seed=5, stride=7)[1] is None
    wrong_count = lambda s: right(s)[:2] + (right(s)[2] + 1,)
    assert "n_matches" in FM.exhaustive_check("lm", 2, 2, wrong_count, seed=5)[1]


# ---------------------------------------------------------------- planted mismatches
@pytest.mark.parametrize("name", list(FM.FAMILIES))
def test_planted_mismatch_is_reported(name):
    fam = FM.FAMILIES[name]
    rng, planted, names = np.random.default_rng(fam.seed), set(), set()
    for i in range(fam.cases):
        want, _ = fam.reference(fam.draw(rng, i))
        assert FM.compare(want, {k: np.array(v) for k, v in want.items()}) == (True, [])
        names |= set(want)
        for k, v in want.items():
            v = np.asarray(v)
            where = np.nonzero(~np.isnan(v.reshape(-1)))[0] if v.dtype.kind == "f" else np.arange(v.size)      # a NaN only has to meet a NaN
            if k in planted or len(where) == 0:
                continue
            got = {j: np.array(x) for j, x in want.items()}
            flat = got[k].reshape(-1)
            at = int(where[int(rng.integers(0, len(where)))])
            raw = flat[at:at + 1].view(np.uint8)
            raw[0] ^= 1                                                 # one bit of one element: -0.0 for 0.0 and one NaN for another differ too
            good, bad = FM.compare(want, got)
            assert not good and bad == [k], (name, i, k, bad)
            planted.add(k)
    assert planted == names, (name, sorted(names - planted))


# ---------------------------------------------------------------- the generators' defaults
def digest(x):
    h = hashlib.sha256()

    def walk(v):
        if isinstance(v, dict):
            for k in sorted(v, key=str):
                h.update(("k:%s;" % k).encode())
                walk(v[k])
        elif isinstance(v, (list, tuple)):
            h.update(b"[")
            for e in v:
                walk(e)
            h.update(b"]")
        elif isinstance(v, np.ndarray):
            a = np.ascontiguousarray(v)
            h.update(("a:%s:%s;" % (a.dtype.str if a.dtype.names is None else a.dtype.descr, a.shape)).encode())
            h.update(a.tobytes())
        elif isinstance(v, np.generic):
            walk(np.asarray(v))
        else:
            h.update(("s:%r;" % (v,)).encode())
    walk(x)
    return h.hexdigest()[:16]


def _defaults():
    from test_gpu_landmark_descriptors import ragged_batch
    T9 = KC.random_table(9, 800, 300)
    return {
        "track.replay_state(77063,63,65)": TC.replay_state(77063, 63, 65),
        "track.replay_state(130003,130,130)": TC.replay_state(130003, 130, 130),
        "refkf.replay_state(88130,130)": RC.replay_state(88130, 130),
        "kfgraph.random_table(7,64,3000,40,big)": KC.random_table(7, 64, 3000, max_obs=40, big=[(11, 64)]),
        "kfgraph.random_table(9,800,300,window)": KC.random_table(9, 800, 300, window=True),
        "kfgraph.random_candidates(9,T9,[0,1,63])": KC.random_candidates(9, T9, [0, 1, 63]),
        "landmark_entry.random_batch(3,200)": LE.random_batch(3, 200),
        "landmark_entry.random_batch(4,50,special=False)": LE.random_batch(4, 50, special=False),
        "ragged_batch(7,200,big)": ragged_batch(7, 200, big=[(5, 90)]),
        "place.random_scene(5,64,1000)": PL.random_scene(5, 64, 1000),
        "place.random_scene(2,2,1000)": PL.random_scene(2, 2, 1000, n_queries=2),
        "localmap.random_keyframes(4,300)": LM.random_keyframes(4, 300),
        "localmap.random_points(4,50,400)": LM.random_points(4, 50, 400),
        "keyframe.seeded(7763,63)": KF.seeded(7763, 63),
        "keyframe.seeded(5,200,sensor=0)": KF.seeded(5, 200, sensor=0),
    }


# sha256 (first 16 hex digits) of the cases above, computed on the commit before the generators took density parameters
DIGESTS = {
    "track.replay_state(77063,63,65)": "decfb0a350fa91a8",
    "track.replay_state(130003,130,130)": "3a958ccb41a5a084",
    "refkf.replay_state(88130,130)": "67460d57a68b8aba",
    "kfgraph.random_table(7,64,3000,40,big)": "f7778ac25ab36329",
    "kfgraph.random_table(9,800,300,window)": "ac201d3e8f590337",
    "kfgraph.random_candidates(9,T9,[0,1,63])": "b562ebec75c71d12",
    "landmark_entry.random_batch(3,200)": "e0817c1a7e4137c1",
    "landmark_entry.random_batch(4,50,special=False)": "ebc75806cff739b2",
    "ragged_batch(7,200,big)": "17fe26c8c9f194e9",
    "place.random_scene(5,64,1000)": "8e4a9db664a27abc",
    "place.random_scene(2,2,1000)": "65ec8a5f44812c62",
    "localmap.random_keyframes(4,300)": "97d4557721ca91ba",
    "localmap.random_points(4,50,400)": "ce00b46b1ad0a63a",
    "keyframe.seeded(7763,63)": "abc269d8d6278574",
    "keyframe.seeded(5,200,sensor=0)": "614c316d4ef832a7",
}


def test_generators_with_default_parameters_are_unchanged():
    got = {k: digest(v) for k, v in _defaults().items()}
    assert got == DIGESTS, {k: (got[k], DIGESTS[k]) for k in DIGESTS if got[k] != DIGESTS[k]}
