"""What the -m gpu tests of the resident chain compare and how (tests/test_gpu_track.py, tests/test_gpu_keyframe.py, tests/test_gpu_chain_run.py):
the fields a call defines completely, two results byte for byte, a tracking result against tests/ref_track.py (integers exactly, Tcw_d within TAU,
DESIGN.md 5.11) and a key-frame result against tests/ref_keyframe.py."""
import numpy as np

import ref_track as R

TAU = 2.1e-9            # the bound on |Tcw_d - reference| for a qualified problem


# fields whose bytes a call defines completely (edge and flag arrays are written up to the count only: compared up to it)
WHOLE = ("pose_view", "problem", "last_lms", "narrow_idx", "narrow_dist", "narrow_n", "wide_idx", "wide_dist", "wide_n", "op_view", "n_edges_motion", "pose_motion",
         "n_edges_local", "pose_local", "result", "kp_lm", "kp_outl", "n_matches", "kp_lm_obs", "local.weights", "local.max_slot", "local.max_count", "local.local",
         "local.n_local", "local.frame_remove", "local.sel", "local.n_sel", "local.lms", "local.match_idx", "local.match_dist", "local.n_matches")


def same_outputs(a, b, what):
    for k in WHOLE:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)
    for stage in ("motion", "local"):
        ne = int(a["n_edges_" + stage][0])
        assert a["edges_" + stage][:ne].tobytes() == b["edges_" + stage][:ne].tobytes(), (what, stage)
        run = int(a["n_edges_motion"][1]) if stage == "motion" else ne
        if run >= 3:
            assert a["outlier_" + stage][:run].tobytes() == b["outlier_" + stage][:run].tobytes(), (what, stage)


def compare_stage(got, ref, stage, c, report):
    """one stage's device outputs against the reference's: integers exactly, Tcw_d within TAU.  -> True when the float pose has the reference's bytes"""
    pose = got["pose_" + stage][0]
    ne = ref["n_edges"]
    assert int(got["n_edges_" + stage][0]) == ne
    assert got["edges_" + stage][:ne].tobytes() == np.ascontiguousarray(ref["edges"]).tobytes(), stage
    rp = ref["pose"]
    print("%s %s: |Tcw_d - ref| = %.3g" % (report, stage, float(np.abs(pose["Tcw_d"].reshape(4, 4) - rp["Tcw_d"]).max())))
    assert (int(pose["status"]), int(pose["n_edges"]), int(pose["n_good"]), int(pose["rounds"])) == (rp["status"], rp["n_edges"], rp["n_good"], rp["rounds"]), stage
    assert np.abs(pose["Tcw_d"].reshape(4, 4) - rp["Tcw_d"]).max() <= TAU, stage
    if rp["status"] != 1:
        assert np.array_equal(got["outlier_" + stage][:ne], rp["outlier"]), stage
    return pose["Tcw"].tobytes() == np.ascontiguousarray(rp["Tcw"], np.float32).tobytes()


def compare_track(got, c, ref, report, LM_DTYPE):
    """every output of hs_track_frame_device (`got`: field -> array, the state included) against the reference chain: integers exactly, Tcw_d within TAU"""
    motion, local = ref
    assert got["pose_view"][0].tobytes() == motion["pose_view"].tobytes()
    assert got["last_lms"].tobytes() == np.ascontiguousarray(motion["last_lms"], LM_DTYPE).tobytes()
    for k in ("narrow_idx", "narrow_dist", "wide_idx", "wide_dist", "op_view"):
        assert got[k].tobytes() == motion[k].tobytes(), k
    r = got["result"][0]
    assert (int(r["status"]), int(r["used_wide"]), int(r["n_narrow"]), int(r["n_wide"])) == (motion["status"], motion["used_wide"], motion["narrow_n"], motion["wide_n"])
    assert (int(got["narrow_n"][0]), int(got["wide_n"][0])) == (motion["narrow_n"], motion["wide_n"])
    assert got["n_edges_motion"].tolist() == [motion["n_edges"], motion["n_edges_run"]]
    same_pose = compare_stage(got, motion, "motion", c, report)
    assert int(r["n_matches_map"]) == motion["n_matches_map"]
    if not same_pose:                                           # the float pose is a rounding of a double that may differ by 1e-10: the reference's
        print(report + ": the device's float pose differs from the reference's; stage 2 is compared from the device's pose")      # stage 2 from the DEVICE's pose
        local = R.track_local_map(c["frame"], got["pose_motion"][0]["Tcw"].reshape(4, 4), c["T"], c["lms"], c["neigh"], c["parent"], c["cap"], c["tp"],
                                  R.DenseMatches.from_dense(*motion["state"]))
    assert got["pose_view"][1].tobytes() == local["pose_view"].tobytes()
    for k in ("weights", "local", "frame_remove", "sel", "match_idx", "match_dist"):
        assert np.array_equal(got["local." + k], local[k]), k
    assert (int(got["local.max_slot"][0]), int(got["local.max_count"][0]), int(got["local.n_local"][0]), int(got["local.n_sel"][0]), int(got["local.n_matches"][0])) == \
        (local["max_slot"], local["max_count"], local["n_local"], local["n_sel"], local["n_matches"])
    assert got["local.lms"].tobytes() == np.ascontiguousarray(local["lms"], LM_DTYPE).tobytes()
    compare_stage(got, local, "local", c, report)
    assert int(r["n_inliers"]) == local["n_inliers"]
    for g, w, what in zip((got["kp_lm"], got["kp_outl"], int(got["n_matches"][0])), local["state"], ("kp_lm", "kp_outl", "n_matches")):
        assert np.array_equal(g, w), what
    return got


def compare_keyframe(got, want, new_cap, tag, stages=range(1, 7), behind=0x55):
    """the key-frame stages' outputs against ref_keyframe: the result keys, the state, the records up to min(n_new, new_cap); `behind`: the byte the
    buffers were filled with, which the records behind the last one must still hold (None: not checked here)"""
    r = got["result"][0]
    fields = {1: ("ref_slot",), 2: ("ok",), 3: ("n_valid",), 4: ("n_ref_matches", "n_tracked_close", "n_nontracked_close", "insert"),
              5: ("n_new", "n_candidates", "n_processed"), 6: ()}
    for s in stages:
        for k in fields[s]:
            assert int(r[k]) == want["result"][k], (tag, k, int(r[k]), want["result"][k])
    assert got["ref_slot_mem"] == want["result"]["ref_slot"], tag
    for k in ("kp_lm", "kp_outl", "n_matches", "kp_lm_obs"):
        assert np.array_equal(got[k], want[k]), (tag, k, got[k], want[k])
    if 5 not in stages:
        return
    assert got["pose_view"].tobytes() == np.asarray(want["pose_view"]).tobytes(), (tag, "pose_view")
    m = min(want["result"]["n_new"], new_cap)
    assert np.array_equal(got["new_view"][:m], want["new_view"][:m]), (tag, "new_view")
    assert got["new_pos"].reshape(-1, 3)[:m].tobytes() == want["new_pos"][:m].tobytes(), (tag, "new_pos")
    assert got["entries"][:m].tobytes() == want["entries"].tobytes() and got["obs"][:m].tobytes() == want["obs"].tobytes(), (tag, "records")
    assert got["desc"].reshape(-1, 32)[:m].tobytes() == want["desc"].tobytes(), (tag, "desc")
    assert np.array_equal(got["lm_index"], want["lm_index"]), (tag, "lm_index")
    assert np.array_equal(got["obs_offsets"], want["offsets"]) and np.array_equal(got["desc_offsets"], want["offsets"]), (tag, "offsets")
    if behind is None:
        return
    for k in ("new_view", "new_pos", "entries", "obs", "desc"):                 # nothing behind the last record
        tail = got[k].view(np.uint8).reshape(new_cap, -1)[m:] if new_cap else np.zeros(0, np.uint8)
        assert (tail == behind).all(), (tag, k, "written behind n_new")
