"""CPU: tests/ref_keyframe.py's two restatements of the stages after the track functions — the reference's own control flow on std::maps (literal)
and the kernels' algorithm on the device layout (dense) — agree on an exhaustive small space, on the directed cases of tests/keyframe_cases.py (each
with a witness that its edge occurred) and on seeded cases; every mutation of the closed form is caught by a named case; UnprojectStereo is within
1 ulp of a float64 evaluation and bit-identical to a second evaluation of the stated rounding order."""
import itertools

import numpy as np
import pytest

import keyframe_cases as KC
import ref_keyframe as RKF
import ref_track as R

DEPTHS = (10.0, KC.TH, 50.0, -1.0)                              # near (twice in a pattern: a tie), th_depth itself, far, a value <= 0
TABLES = [(nobs, bad) for nobs in itertools.product((0, 1), repeat=3) for bad in itertools.product((0, 1), repeat=3)]
VIEW_KINDS = [(lm, o) for lm in (-1, 0, 1, 2) for o in (0, 1, 2)]       # every association with every flag, stale flags on empty views included


def _check(c, tag):
    a, b = RKF.literal(c), RKF.dense(c)
    assert RKF.same(a, b) is None, (tag, RKF.same(a, b))
    return a


def depth_pattern_cases():
    """up to 5 views: every depth pattern x every n_min_points, the associations and the landmark table cycling through all of theirs"""
    for n in range(1, 6):
        for k, depth in enumerate(itertools.product(DEPTHS, repeat=n)):
            for nmp in range(4):
                kinds = [VIEW_KINDS[(k * 7 + nmp * 5 + 5 * i) % 12] for i in range(n)]
                nobs, bad = TABLES[(k + 3 * nmp) % 64]
                yield (depth, nmp, kinds, nobs, bad), KC.make(depth, [v[0] for v in kinds], [v[1] for v in kinds], lm_nobs=nobs, lm_bad=bad, n_min_points=nmp)


def association_cases():
    """up to 3 views: every (association, flag) pattern x every lm_nobs pattern, lm_bad / depths / n_min_points cycling"""
    for n in range(1, 4):
        for k, kinds in enumerate(itertools.product(VIEW_KINDS, repeat=n)):
            for t, nobs in enumerate(itertools.product((0, 1), repeat=3)):
                bad = TABLES[(k + t) % 64][1]
                depth = [DEPTHS[(k + t + 3 * i) % 4] for i in range(n)]
                yield (kinds, nobs, bad, depth), KC.make(depth, [v[0] for v in kinds], [v[1] for v in kinds], lm_nobs=nobs, lm_bad=bad, n_min_points=(k + t) % 4)


def table_cases():
    """two views: every association pattern x every (lm_nobs, lm_bad) table x both gates"""
    for lms in itertools.product((-1, 0, 1, 2), repeat=2):
        for t, (nobs, bad) in enumerate(TABLES):
            for ok in (0, 1):
                yield (lms, nobs, bad, ok), KC.make([10.0, 50.0], lms, [1 + (t & 1), 2 - (t & 1)], lm_nobs=nobs, lm_bad=bad, ok_override=ok, n_min_points=t % 3)


def exhaustive_cases():
    """the three spaces one after the other (22 576 cases): what tools/fuzz_map.py and tests/test_gpu_fuzz_map.py run on the device"""
    for cases in (depth_pattern_cases, association_cases, table_cases):
        yield from cases()


def test_exhaustive_depth_patterns():
    count, inserted, cut = 0, 0, 0
    for tag, c in depth_pattern_cases():
        r = _check(c, tag)
        count += 1
        inserted += r["result"]["n_new"] > 0
        cut += r["result"]["n_processed"] < r["result"]["n_candidates"]
    assert count == 4 * sum(4 ** n for n in range(1, 6)) and inserted > 1000 and cut > 200


def test_exhaustive_associations():
    count = 0
    for tag, c in association_cases():
        _check(c, tag)
        count += 1
    assert count == 8 * (12 + 144 + 1728)


def test_exhaustive_tables_on_two_views():
    count = 0
    for tag, c in table_cases():
        _check(c, tag)
        count += 1
    assert count == 16 * 64 * 2


@pytest.mark.parametrize("name", sorted(KC.DIRECTED))
def test_directed(name):
    c, witness = KC.DIRECTED[name]
    r = _check(c, name)
    assert witness(r), (name, r["result"], r["kp_lm"], r["kp_outl"], r["n_matches"], r["new_view"])


@pytest.mark.parametrize("n", [1, 7, 64, 200])
def test_seeded(n):
    for seed in range(8):
        _check(KC.seeded(9100 + seed, n), (n, seed))


def test_gpu_seeded_cases_reach_every_branch():
    """what the seeded cases of tests/test_gpu_keyframe.py cover: insert and no insert, a cut walk and a whole one, truncated records, stage-3 removals"""
    seen = dict(insert=0, no_insert=0, cut=0, whole=0, removed_unobserved=0, truncated=0, roomy=0)
    for n in KC.GPU_SIZES[1:]:
        for seed in range(8):
            c = KC.gpu_seeded(n, seed)
            r = RKF.dense(c)["result"]
            seen["insert"] += r["insert"]
            seen["no_insert"] += not r["insert"]
            seen["cut"] += r["n_processed"] < r["n_candidates"]
            seen["whole"] += r["insert"] and r["n_processed"] == r["n_candidates"]
            seen["truncated"] += c["new_cap"] < r["n_new"]
            seen["roomy"] += c["new_cap"] > r["n_new"] > 0
            seen["removed_unobserved"] += RKF.dense(c, stages=(1, 2, 3))["n_matches"] < RKF.dense(c, stages=(1, 2))["n_matches"]
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("n", KC.GPU_SIZES)
def test_gpu_seeded_cases_literal_equals_dense(n):
    """the reference of tests/test_gpu_keyframe.py's seeded cases is the sequential walk at every size, 1025 and 2049 included"""
    for seed in range(8):
        _check(KC.gpu_seeded(n, seed), (n, seed))


def test_single_stages_compose():
    """the stages run one by one, each from the state and the result the previous one left, give the composite's result"""
    for seed in range(6):
        c = KC.seeded(9300 + seed, 40, force=1)
        whole, cur, res = RKF.literal(c), dict(c), None
        for s in range(1, 7):
            for f in (RKF.literal, RKF.dense):
                r = f(cur, stages=(s,), res=res)
            cur = dict(cur, state=(r["kp_lm"], r["kp_outl"], r["n_matches"]), ref_slot=r["result"]["ref_slot"])
            res = r["result"]
            if s == 5:
                made = r
        assert res == whole["result"] and r["kp_lm"].tobytes() == whole["kp_lm"].tobytes() and r["n_matches"] == whole["n_matches"]
        assert made["new_pos"].tobytes() == whole["new_pos"].tobytes()


# which directed case catches which mutation of the closed form (the first named is enough; the exhaustive space catches all of them too)
CAUGHT_BY = dict(ge_th="depth_equals_th_depth", tie_desc="equal_depths", overwrite_stale="empty_stale_flag_2", no_max="far_before_n_min_points",
                 outlier_tracked="outlier_not_tracked_close")


@pytest.mark.parametrize("mut", RKF.MUTATIONS)
def test_mutations_are_caught(mut):
    c, _ = KC.DIRECTED[CAUGHT_BY[mut]]
    assert RKF.same(RKF.literal(c), RKF.dense(c, mut=mut)) is not None, mut
    caught = [name for name, (c, _) in sorted(KC.DIRECTED.items()) if RKF.same(RKF.literal(c), RKF.dense(c, mut=mut)) is not None]
    assert CAUGHT_BY[mut] in caught
    print(mut, "caught by", caught)


def _unproject_again(u, v, z, fr, pv):
    """the stated rounding order, written independently: float32 camera step, float64 dot product of a row of Rwc = Rcw^T, + Ow, one rounding"""
    f4, f8 = np.float32, np.float64
    with np.errstate(all="ignore"):
        x3 = np.array([(f4(u) - f4(fr["cx"])) * (f4(z) / f4(fr["fx"])), (f4(v) - f4(fr["cy"])) * (f4(z) / f4(fr["fy"])), f4(z)], f4)
        Rwc = pv["Rcw"].reshape(3, 3).T.astype(f8)
        out = []
        for r in range(3):
            acc = f8(0)
            for col in range(3):
                acc = acc + Rwc[r, col] * f8(x3[col])
            out.append(f4(acc + f8(pv["Ow"][r])))
    return np.array(out, f4)


def test_unproject_stereo():
    rng = np.random.default_rng(5)
    fr = KC.frame(1)
    for seed in range(200):
        pv = R.pose_view(KC.pose(seed))
        u, v, z = np.float32(rng.uniform(0, 1240)), np.float32(rng.uniform(0, 370)), np.float32(rng.uniform(0.3, 120))
        got = RKF.unproject_stereo(u, v, z, fr, pv)
        assert got.tobytes() == _unproject_again(u, v, z, fr, pv).tobytes()
        # the issue's check: a float64 evaluation of Rwc * x3Dc + Ow from the same float-rounded x3Dc, within 1 ulp of float
        with np.errstate(all="ignore"):
            x3 = np.array([np.float32(np.float32(u - np.float32(fr["cx"])) * np.float32(z / np.float32(fr["fx"]))),
                           np.float32(np.float32(v - np.float32(fr["cy"])) * np.float32(z / np.float32(fr["fy"]))), z], np.float64)
        ref64 = pv["Rcw"].reshape(3, 3).T.astype(np.float64) @ x3 + pv["Ow"].astype(np.float64)
        ulp = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - ref64) <= ulp).all(), (seed, got, ref64)
        # beside it, a sanity bound against float64 THROUGHOUT (the camera step in double as well), from the same float inputs: the float camera step contributes a few ulp of x and y, scaled by |R| <= 1
        x = (float(u) - float(np.float32(fr["cx"]))) * (float(z) / float(np.float32(fr["fx"])))
        y = (float(v) - float(np.float32(fr["cy"]))) * (float(z) / float(np.float32(fr["fy"])))
        exact = pv["Rcw"].reshape(3, 3).T.astype(np.float64) @ np.array([x, y, float(z)]) + pv["Ow"].astype(np.float64)
        # x and y carry 3 float roundings each (<= 1.5 ulp relative), the gemm adds half an ulp of the result
        bound = 1.5 * np.finfo(np.float32).eps * (abs(x) + abs(y)) + np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - exact) <= bound).all(), (seed, got, exact)
    for z in (np.float32(np.inf), np.float32(1e-30)):
        pv = R.pose_view(KC.pose(1))
        assert RKF.unproject_stereo(5.0, 6.0, z, fr, pv).tobytes() == _unproject_again(5.0, 6.0, z, fr, pv).tobytes() or np.isnan(RKF.unproject_stereo(5.0, 6.0, z, fr, pv)).any()
