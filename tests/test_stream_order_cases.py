"""CPU: the (real, decoy) pairs of tests/stream_order_cases.py.  A pair that cannot tell a late input from an early one is rejected HERE, not on the GPU:
the two cases have equal shapes and dtypes, every primary output of the real case differs from the decoy's (references only: nothing runs on a device),
and what the kernels trust on the device — CSR offsets, indices, counts — is valid in BOTH, so that no order of execution reads out of range."""
import numpy as np
import pytest

import stream_order_cases as S


@pytest.fixture(scope="module")
def cases():
    return S.single_cases()


def differs(segs):
    return any(np.ascontiguousarray(r).tobytes() != np.ascontiguousarray(d).tobytes() for _, r, d in segs)


def check_case(c):
    assert c.inputs or getattr(c, "link", None), c
    for k, (r, d) in c.inputs.items():
        assert r.shape == d.shape and r.dtype == d.dtype and r.flags.c_contiguous and d.flags.c_contiguous, (c, k)
        assert r.tobytes() != d.tobytes() or k == "T.lm_obs_offsets" or r.size == 0, (c, k, "the decoy input equals the real one")
    assert not set(c.inputs) & set(c.outputs), (c, "an input and an output of one name would share a buffer")
    for k, segs in c.expect.items():
        assert k in c.outputs, (c, k)
        for off, r, d in segs:
            assert r.dtype == d.dtype, (c, k)
            assert off + max(np.ascontiguousarray(r).nbytes, np.ascontiguousarray(d).nbytes) <= c.outputs[k], (c, k, "defined bytes behind the output")
    for k in c.primary:
        assert differs(c.expect[k]), (c, k, "the real and the decoy result are the same: the pair cannot tell them apart")
    if "T.lm_obs_offsets" in c.inputs:
        for which in (0, 1):
            S.valid_table(c.inputs, which)


def test_every_pair_has_equal_shapes_and_different_results(cases):
    kinds = {c.kind for c in cases}
    assert kinds >= {"extract_batch", "stereo_frontend", "stereo_match", "preprocess", "projection", "projection_posed", "hamming_knn2", "records_knn2",
                     "records_bow_match", "bow_transform", "bow_vector", "landmark_best_descriptors", "kf_votes", "kf_redundancy", "local_keyframes",
                     "local_points", "landmark_gather", "local_map_search", "pose_edges", "pose_optimize"}
    for c in cases:
        check_case(c)


def test_device_trusted_values_are_valid_in_both_cases(cases):
    by = {(c.kind, c.name): c for c in cases}
    for which in (0, 1):
        for path in ("small", "large"):
            c = by["landmark_best_descriptors", path]
            off = c.inputs["offsets"][which]
            assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(c.inputs["desc"][which])
        assert np.diff(by["landmark_best_descriptors", "small"].inputs["offsets"][which]).max() <= 64 < np.diff(by["landmark_best_descriptors", "large"].inputs["offsets"][which]).max()
        for name in ("lds", "global"):
            c = by["kf_votes", name]
            off, q = c.inputs["q_offsets"][which], c.inputs["q_lm"][which]
            assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(q) and q.min() >= 0 and q.max() < c.args["L"]
        c = by["kf_redundancy", "five"]
        off = c.inputs["cand_offsets"][which]
        assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(c.inputs["item_lm"][which])
        assert c.inputs["item_lm"][which].max() < c.args["L"] and 0 <= c.inputs["cand_slot"][which].min() and c.inputs["cand_slot"][which].max() < c.args["n_kf"]
        c = by["local_keyframes", "129"]
        for k in ("neigh", "parent"):
            assert c.inputs[k][which].min() >= -1 and c.inputs[k][which].max() < c.args["n_kf"]
        c = by["local_points", "3blocks+1"]
        assert c.inputs["frame_lm"][which].min() >= -1 and c.inputs["frame_lm"][which].max() < c.args["L"]
        c = by["landmark_gather", "37of64"]
        n = int(c.inputs["n_sel"][which][0])
        assert 0 <= n <= c.args["cap"] and c.inputs["sel"][which][:n].min() >= 0 and c.inputs["sel"][which][:n].max() < c.args["L"]
        c = by["local_map_search", "640x480"]
        assert c.inputs["frame_lm"][which].max() < c.args["L"] and c.inputs["neigh"][which].max() < c.args["n_kf"] and c.inputs["parent"][which].max() < c.args["n_kf"]
        assert c.inputs["map_lms"][which]["assoc_kp"].max() < len(c.inputs["F.kps"][which])
        c = by["pose_optimize", "n257"]
        assert 3 <= int(c.inputs["n_edges"][which][0]) <= c.args["cap"]
        c = by["stereo_match", "3 pairs"]
        assert c.inputs["nL"][which].max() <= c.args["cap"] and c.inputs["nR"][which].max() <= c.args["cap"]
        for c in cases:
            if c.kind in ("bow_transform", "bow_vector"):
                assert 0 <= int(c.inputs["n"][which][0]) <= c.args["n_max"]
    # the two vote cases sit on either side of the LDS limit
    from hyslam_amd import _native as N
    assert by["kf_votes", "lds"].args["n_kf"] <= N.HS_KF_LDS_SLOTS < by["kf_votes", "global"].args["n_kf"]


def test_place_scene():
    sc = S.place_scene()
    assert [c.kind for c in sc["steps"]] == ["place_add", "place_add", "place_query_reloc", "place_query_loop"]
    for c in sc["steps"]:
        check_case(c)
        for which in (0, 1):
            if c.kind == "place_add":
                m, w = int(c.inputs["m"][which][0]), c.inputs["word"][which]
                assert 0 < m <= c.args["m_max"] and (np.diff(w[:m]) > 0).all() and w[:m].max() < sc["n_words"] and (c.inputs["value"][which][:m] > 0).all()
            else:
                m, w = int(c.inputs["qm"][which][0]), c.inputs["qword"][which]
                assert 0 < m <= c.args["qm_max"] and (np.diff(w[:m]) > 0).all() and w[:m].max() < sc["n_words"]
                assert c.inputs["neigh"][which].min() >= -1 and c.inputs["neigh"][which].max() < c.args["slots"]
                assert int(c.expect["n_cand"][0][1 + which][0]) >= 1
    # a query tells whether the device-added vectors had arrived: its real result names a slot the stream added
    assert int(sc["steps"][2].expect["cand"][0][1][0]) >= len(sc["host"])


def test_chain_scene():
    sc = S.chain_scene(S.CPU_CAP)
    assert [c.kind for c in sc["steps"]] == ["extract_batch", "bow_transform", "bow_vector", "place_add", "place_query_reloc"]
    for i, c in enumerate(sc["steps"]):
        check_case(c)
        for k, (j, out) in c.link.items():
            assert j < i and out in sc["steps"][j].outputs, (c, k)
        for k, a in c.prefill.items():                            # the intermediate buffers start from the decoy's result
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(c.expect[k][0][2]).tobytes(), (c, k)
    linked = {(j, out) for c in sc["steps"] for j, out in c.link.values()}
    assert all(out in sc["steps"][j].prefill for j, out in linked if out not in ("node",)), "a linked buffer that starts from 0x55 is no valid decoy"
    m = sc["steps"][2].expect["m"][0]
    assert 0 < int(m[1][0]) <= S.CPU_CAP and 0 < int(m[2][0]) <= S.CPU_CAP and sc["steps"][2].expect["out_word"][0][1].max() < sc["n_words"]
