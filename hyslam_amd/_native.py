"""ctypes binding of libhyslam_amd.so (the C ABI in include/hyslam_amd.h).

There is no CPU fallback: if the HIP library is missing or cannot be loaded this module raises.
"""
import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# HYSLAM_AMD_LIB: development only — an instrumented build of the same sources (make BUILD=_build_prof OUT=../libhyslam_amd_prof.so EXTRA=-D...)
LIB_PATH = os.environ.get("HYSLAM_AMD_LIB") or os.path.join(_HERE, "libhyslam_amd.so")

HS_OK, HS_ERR_INVALID, HS_ERR_HIP, HS_ERR_CAPACITY, HS_ERR_NO_DEVICE, HS_ERR_POISON = 0, 1, 2, 3, 4, 5

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32), ("cell_px", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32), ("fast_threshold", C.c_int32),
                ("blur_taps", C.c_uint16 * 7), ("_pad", C.c_uint16)]


class PreprocessParams(C.Structure):
    _fields_ = [("channels", C.c_int32), ("rgb", C.c_int32), ("scale", C.c_float), ("_pad", C.c_int32)]


class StereoParams(C.Structure):
    _fields_ = [("fx", C.c_float), ("mbf", C.c_float), ("n_rows", C.c_int32), ("th_high", C.c_float),
                ("th_low", C.c_float), ("size_ref", C.c_float)]


LM_DTYPE = np.dtype([("pos", "<f4", 3), ("size", "<f4"), ("min_dist", "<f4"), ("max_dist", "<f4"), ("normal", "<f4", 3),
                     ("assoc_kp", "<i4"), ("prev_angle", "<f4"), ("skip", "<i4"), ("desc", "u1", 32)])


# hs_lm_entry_in / hs_lm_obs (include/hyslam_amd.h): the landmark entry update's per-landmark and per-observation records
LM_ENTRY_DTYPE = np.dtype([("pos", "<f4", 3), ("ref_Ow", "<f4", 3)])
LM_OBS_DTYPE = np.dtype([("Ow", "<f4", 3), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("u", "<f4"), ("v", "<f4"),
                         ("kp_size", "<f4"), ("assoc_pos", "<f4", 3), ("assoc", "<i4")])
HS_LM_SET_NORMAL_DEPTH, HS_LM_SET_DESC, HS_LM_SET_MEAN, HS_LM_SET_SIZE = 1, 2, 4, 8


class LmEntryParams(C.Structure):
    _fields_ = [("max_dist_factor", C.c_float), ("min_dist_factor", C.c_float)]

    def __init__(self, max_dist_factor=2.0, min_dist_factor=0.5):
        super().__init__(max_dist_factor, min_dist_factor)


# hs_kf_table (include/hyslam_amd.h): the observation table of the key-frame graph entry points; host or device pointers
class KfTable(C.Structure):
    _fields_ = [("L", C.c_int32), ("n_kf", C.c_int32), ("lm_obs_offsets", C.c_void_p), ("lm_obs_kf", C.c_void_p), ("lm_obs_octave", C.c_void_p),
                ("lm_bad", C.c_void_p), ("lm_nobs", C.c_void_p), ("kf_bad", C.c_void_p), ("kf_id", C.c_void_p)]


def _header_constant(name):
    """the value of `#define name <integer>` in include/hyslam_amd.h: the header is the one place that states it"""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hyslam_amd.h")) as f:
        m = re.search(r"^#define[ \t]+%s[ \t]+(\d+)[ \t]*$" % name, f.read(), re.M)
    if not m:
        raise ImportError("include/hyslam_amd.h does not define " + name)
    return int(m.group(1))


HS_KF_LDS_SLOTS, HS_KF_SORT_PASS = _header_constant("HS_KF_LDS_SLOTS"), _header_constant("HS_KF_SORT_PASS")
HS_LOCAL_POINTS_BLOCK = _header_constant("HS_LOCAL_POINTS_BLOCK")


# hs_local_map_out (include/hyslam_amd.h): the device outputs of hs_local_map_search_device
class LocalMapOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("weights", "max_slot", "max_count", "local", "n_local", "frame_remove", "sel", "n_sel", "lms", "match_idx",
                                          "match_dist", "n_matches")]


# hs_pose_edge / hs_pose_problem / hs_pose_result (include/hyslam_amd.h): the pose-only optimisation
POSE_EDGE_DTYPE = np.dtype([("Xw", "<f4", 3), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("inv_sigma2", "<f4"), ("kp", "<i4")])
POSE_PROBLEM_DTYPE = np.dtype([("Tcw", "<f4", 16), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("bf", "<f4")])
POSE_RESULT_DTYPE = np.dtype([("Tcw_d", "<f8", 16), ("Tcw", "<f4", 16), ("n_edges", "<i4"), ("n_good", "<i4"), ("rounds", "<i4"),
                              ("lm_iterations", "<i4"), ("lm_trials", "<i4"), ("status", "<i4")])
HS_POSE_OK, HS_POSE_TOO_FEW, HS_POSE_NONFINITE = 0, 1, 2


class PoseEdge(C.Structure):
    _fields_ = [("Xw", C.c_float * 3), ("u", C.c_float), ("v", C.c_float), ("ur", C.c_float), ("inv_sigma2", C.c_float), ("kp", C.c_int32)]


class PoseProblem(C.Structure):
    _fields_ = [("Tcw", C.c_float * 16), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float)]


class PoseResult(C.Structure):
    _fields_ = [("Tcw_d", C.c_double * 16), ("Tcw", C.c_float * 16), ("n_edges", C.c_int32), ("n_good", C.c_int32), ("rounds", C.c_int32),
                ("lm_iterations", C.c_int32), ("lm_trials", C.c_int32), ("status", C.c_int32)]


# hs_pnp_* (include/hyslam_amd.h): relocalisation, EPnP inside RANSAC
PNP_CORR_DTYPE = np.dtype([("Xw", "<f4", 3), ("u", "<f4"), ("v", "<f4"), ("sigma2", "<f4"), ("kp", "<i4"), ("_pad", "<i4")])
PNP_PARAMS_DTYPE = np.dtype([("probability", "<f8"), ("min_inliers", "<i4"), ("max_iterations", "<i4"), ("min_set", "<i4"), ("epsilon", "<f4"), ("th2", "<f4"),
                             ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("_pad", "<i4"), ("seed", "<u8")])
PNP_STATE_DTYPE = np.dtype([("iterations", "<i4"), ("best_inliers", "<i4"), ("best_Tcw", "<f4", 16)])
PNP_RESULT_DTYPE = np.dtype([("Tcw_d", "<f8", 16), ("Tcw", "<f4", 16), ("status", "<i4"), ("n_inliers", "<i4"), ("at_iteration", "<i4"), ("iterations", "<i4"),
                             ("hypotheses_run", "<i4"), ("refines_run", "<i4")])
HS_PNP_TOO_FEW, HS_PNP_REFINED, HS_PNP_BEST, HS_PNP_NONE, HS_PNP_NONFINITE = 0, 1, 2, 3, 4
HS_PNP_MAX_SET = _header_constant("HS_PNP_MAX_SET")


class PnpCorr(C.Structure):
    _fields_ = [("Xw", C.c_float * 3), ("u", C.c_float), ("v", C.c_float), ("sigma2", C.c_float), ("kp", C.c_int32), ("_pad", C.c_int32)]


class PnpParams(C.Structure):
    _fields_ = [("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("min_set", C.c_int32), ("epsilon", C.c_float),
                ("th2", C.c_float), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("_pad", C.c_int32), ("seed", C.c_uint64)]


class PnpPlan(C.Structure):
    _fields_ = [("min_inliers", C.c_int32), ("epsilon", C.c_float), ("max_iterations", C.c_int32), ("_pad", C.c_int32)]


class PnpState(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("best_inliers", C.c_int32), ("best_Tcw", C.c_float * 16)]


class PnpResult(C.Structure):
    _fields_ = [("Tcw_d", C.c_double * 16), ("Tcw", C.c_float * 16), ("status", C.c_int32), ("n_inliers", C.c_int32), ("at_iteration", C.c_int32),
                ("iterations", C.c_int32), ("hypotheses_run", C.c_int32), ("refines_run", C.c_int32)]


# hs_sim3_* (include/hyslam_amd.h): loop closing, Horn's closed form inside RANSAC
SIM3_CORR_DTYPE = np.dtype([("X1c", "<f4", 3), ("sigma2_1", "<f4"), ("X2c", "<f4", 3), ("sigma2_2", "<f4"), ("idx1", "<i4"), ("_pad", "<i4", 3)])
SIM3_PARAMS_DTYPE = np.dtype([("probability", "<f8"), ("min_inliers", "<i4"), ("max_iterations", "<i4"), ("fix_scale", "<i4"), ("_pad", "<i4"),
                              ("fx1", "<f4"), ("fy1", "<f4"), ("cx1", "<f4"), ("cy1", "<f4"), ("fx2", "<f4"), ("fy2", "<f4"), ("cx2", "<f4"), ("cy2", "<f4"),
                              ("seed", "<u8")])
SIM3_STATE_DTYPE = np.dtype([("iterations", "<i4"), ("best_inliers", "<i4"), ("R", "<f4", 9), ("t", "<f4", 3), ("s", "<f4"), ("T12", "<f4", 16), ("_pad", "<i4")])
SIM3_RESULT_DTYPE = np.dtype([("T12", "<f4", 16), ("R", "<f4", 9), ("t", "<f4", 3), ("s", "<f4"), ("status", "<i4"), ("n_inliers", "<i4"), ("at_iteration", "<i4"),
                              ("iterations", "<i4"), ("hypotheses_run", "<i4")])
HS_SIM3_TOO_FEW, HS_SIM3_FOUND, HS_SIM3_CONTINUE, HS_SIM3_EXHAUSTED, HS_SIM3_NONFINITE = 0, 1, 2, 3, 4
HS_SIM3_DRAW_STRIDE = _header_constant("HS_SIM3_DRAW_STRIDE")


class Sim3Corr(C.Structure):
    _fields_ = [("X1c", C.c_float * 3), ("sigma2_1", C.c_float), ("X2c", C.c_float * 3), ("sigma2_2", C.c_float), ("idx1", C.c_int32), ("_pad", C.c_int32 * 3)]


class Sim3Params(C.Structure):
    _fields_ = [("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("fix_scale", C.c_int32), ("_pad", C.c_int32),
                ("fx1", C.c_float), ("fy1", C.c_float), ("cx1", C.c_float), ("cy1", C.c_float), ("fx2", C.c_float), ("fy2", C.c_float), ("cx2", C.c_float),
                ("cy2", C.c_float), ("seed", C.c_uint64)]


class Sim3Plan(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("epsilon", C.c_float)]


class Sim3State(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("best_inliers", C.c_int32), ("R", C.c_float * 9), ("t", C.c_float * 3), ("s", C.c_float), ("T12", C.c_float * 16),
                ("_pad", C.c_int32)]


class Sim3Result(C.Structure):
    _fields_ = [("T12", C.c_float * 16), ("R", C.c_float * 9), ("t", C.c_float * 3), ("s", C.c_float), ("status", C.c_int32), ("n_inliers", C.c_int32),
                ("at_iteration", C.c_int32), ("iterations", C.c_int32), ("hypotheses_run", C.c_int32)]


# hs_monoinit_* (include/hyslam_amd.h): monocular initialisation, homography / fundamental RANSAC and reconstruction
MONOINIT_PARAMS_DTYPE = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("sigma", "<f4"), ("max_iterations", "<i4"), ("min_triangulated", "<i4"),
                                  ("min_frac_triangulated", "<f4"), ("min_parallax_deg", "<f4"), ("_pad", "<i4"), ("seed", "<u8")])
MONOINIT_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_matches", "<i4"), ("model", "<i4"), ("best_solution", "<i4"), ("best_it_h", "<i4"), ("best_it_f", "<i4"),
                                  ("n_triangulated", "<i4"), ("_pad", "<i4"), ("score_h", "<f4"), ("score_f", "<f4"), ("rh", "<f4"), ("cos_parallax", "<f4"),
                                  ("H21", "<f4", 9), ("F21", "<f4", 9), ("n_good", "<i4", 8), ("R21", "<f4", 9), ("t21", "<f4", 3)])
HS_MONOINIT_TOO_FEW, HS_MONOINIT_FAILED, HS_MONOINIT_OK_H, HS_MONOINIT_OK_F, HS_MONOINIT_NONFINITE = 0, 1, 2, 3, 4
HS_MONOINIT_MODEL_NONE, HS_MONOINIT_MODEL_H, HS_MONOINIT_MODEL_F = 0, 1, 2
HS_MONOINIT_DRAW_STRIDE = _header_constant("HS_MONOINIT_DRAW_STRIDE")
HS_MONOINIT_MAX_ITERATIONS = _header_constant("HS_MONOINIT_MAX_ITERATIONS")


class MonoinitParams(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("sigma", C.c_float), ("max_iterations", C.c_int32),
                ("min_triangulated", C.c_int32), ("min_frac_triangulated", C.c_float), ("min_parallax_deg", C.c_float), ("_pad", C.c_int32), ("seed", C.c_uint64)]


class MonoinitResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_matches", C.c_int32), ("model", C.c_int32), ("best_solution", C.c_int32), ("best_it_h", C.c_int32), ("best_it_f", C.c_int32),
                ("n_triangulated", C.c_int32), ("_pad", C.c_int32), ("score_h", C.c_float), ("score_f", C.c_float), ("rh", C.c_float), ("cos_parallax", C.c_float),
                ("H21", C.c_float * 9), ("F21", C.c_float * 9), ("n_good", C.c_int32 * 8), ("R21", C.c_float * 9), ("t21", C.c_float * 3)]


# hs_pose_view / hs_track_* (include/hyslam_amd.h): frame tracking on resident tables
POSE_VIEW_DTYPE = np.dtype([("Rcw", "<f4", 9), ("tcw", "<f4", 3), ("Ow", "<f4", 3), ("_pad", "<f4")])
TRACK_RESULT_DTYPE = np.dtype([("status", "<i4"), ("used_wide", "<i4"), ("n_narrow", "<i4"), ("n_wide", "<i4"), ("n_matches_map", "<i4"), ("n_inliers", "<i4"),
                               ("_pad", "<i4", 2)])
HS_TRACK_MOTION, HS_TRACK_LOCAL = 0, 1
HS_TRACK_OK, HS_TRACK_MOTION_FAILED = 0, 1


class TrackParams(C.Structure):
    _fields_ = [("th_motion", C.c_float), ("th_motion_wide", C.c_float), ("n_min_matches", C.c_int32), ("th_local", C.c_float), ("nnratio_motion", C.c_float),
                ("nnratio_local", C.c_float), ("th_high", C.c_float), ("sigma_ref", C.c_float), ("n_max_local_keyframes", C.c_int32),
                ("n_neighbor_keyframes", C.c_int32)]

    def __init__(self, th_motion=15.0, th_motion_wide=30.0, n_min_matches=20, th_local=3.0, nnratio_motion=0.9, nnratio_local=0.8, th_high=100.0, sigma_ref=1.0,
                 n_max_local_keyframes=80, n_neighbor_keyframes=10):
        super().__init__(th_motion, th_motion_wide, n_min_matches, th_local, nnratio_motion, nnratio_local, th_high, sigma_ref, n_max_local_keyframes,
                         n_neighbor_keyframes)


class TrackState(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("kp_lm", "kp_outl", "n_matches", "kp_lm_obs")]


# the device outputs of the hs_track_* calls: (field, element dtype or None for a record type, count as a size name or a number)
TRACK_OUT_HEAD = (("pose_view", "pose_view", 2), ("problem", "problem", 2), ("last_lms", "lm", "n_last"), ("narrow_idx", np.int32, "n_last"),
                  ("narrow_dist", np.float32, "n_last"), ("narrow_n", np.int32, 1), ("wide_idx", np.int32, "n_last"), ("wide_dist", np.float32, "n_last"),
                  ("wide_n", np.int32, 1), ("op_view", np.int32, "n_last"), ("edges_motion", "edge", "n"), ("outlier_motion", np.uint8, "n"),
                  ("n_edges_motion", np.int32, 2), ("pose_motion", "result", 1))
TRACK_OUT_TAIL = (("edges_local", "edge", "n"), ("outlier_local", np.uint8, "n"), ("n_edges_local", np.int32, 1), ("pose_local", "result", 1),
                  ("result", "track_result", 1))
LOCAL_MAP_OUT_SPEC = (("weights", np.int32, "n_kf"), ("max_slot", np.int32, 1), ("max_count", np.int32, 1), ("local", np.uint8, "n_kf"), ("n_local", np.int32, 1),
                      ("frame_remove", np.uint8, "n"), ("sel", np.int32, "cap"), ("n_sel", np.int32, 1), ("lms", "lm", "cap"), ("match_idx", np.int32, "cap"),
                      ("match_dist", np.float32, "cap"), ("n_matches", np.int32, 1))


# hs_kf_features (include/hyslam_amd.h): the key frames' features of hs_search_by_bow_kf_device
class KfFeatures(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("kf_off", C.c_void_p), ("kps", C.c_void_p), ("desc", C.c_void_p), ("node", C.c_void_p), ("kp_lm", C.c_void_p), ("weight", C.c_void_p)]


# hs_track_initial_* (include/hyslam_amd.h): initial pose estimation as one resident call
HS_REFKF_OK, HS_REFKF_BOW_FAILED, HS_REFKF_SKIPPED = 0, 1, 2
TRACK_INITIAL_RESULT_DTYPE = np.dtype([("refkf_status", "<i4"), ("n_bow", "<i4"), ("n_matches_map_refkf", "<i4"), ("n_init", "<i4"), ("success", "<i4"),
                                       ("_pad", "<i4", 3)])


class TrackRefkfParams(C.Structure):
    """hs_track_refkf_params; the defaults are the reference's (TrackReferenceKeyFrameParameters, StateNormalParameters)"""
    _fields_ = [("th_low", C.c_float), ("nnratio", C.c_float), ("n_min_matches_bow", C.c_int32), ("thresh_init", C.c_int32)]

    def __init__(self, th_low=50.0, nnratio=0.7, n_min_matches_bow=15, thresh_init=10):
        super().__init__(th_low, nnratio, n_min_matches_bow, thresh_init)


# the device outputs of the hs_track_initial_* calls: (field, element dtype, count as a size name or a number)
TRACK_INITIAL_OUT_SPEC = (("bow_word", np.int32, "n"), ("bow_weight", np.float32, "n"), ("bow_node", np.int32, "n"), ("match_kf", np.int32, "kf_cap"),
                          ("op_view", np.int32, "n"), ("op_lm", np.int32, "n"), ("pose_view", "pose_view", 1), ("problem", "problem", 1), ("edges", "edge", "n"),
                          ("outlier", np.uint8, "n"), ("n_edges", np.int32, 2), ("pose", "result", 1), ("Tcw_init", np.float32, 16),
                          ("result", "track_initial_result", 1), ("frame_result", "track_result", 1))


class TrackInitialOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _, _ in TRACK_INITIAL_OUT_SPEC]


# hs_keyframe_* (include/hyslam_amd.h): reference key frame, key-frame decision, stereo landmark creation
KEYFRAME_RESULT_DTYPE = np.dtype([("ok", "<i4"), ("ref_slot", "<i4"), ("n_valid", "<i4"), ("n_ref_matches", "<i4"), ("n_tracked_close", "<i4"),
                                  ("n_nontracked_close", "<i4"), ("insert", "<i4"), ("n_new", "<i4"), ("n_candidates", "<i4"), ("n_processed", "<i4"),
                                  ("_pad", "<i4", 6)])


class KeyFrameParams(C.Structure):
    """hs_keyframe_params; the defaults are the reference's (Tracking_datastructs.h:103-113), th_depth is the camera's"""
    _fields_ = [("frame_id", C.c_uint64), ("last_keyframe_id", C.c_uint32)] + [(k, C.c_int32) for k in (
        "force", "mapping_stopped", "mapping_idle", "mapping_queue_length", "n_kfs_in_map", "min_N_tracked_close", "thresh_N_nontracked_close", "min_KF_interval",
        "max_KF_interval", "N_tracked_target", "N_tracked_variance")] + [("th_depth", C.c_float)] + [(k, C.c_int32) for k in (
            "n_min_points", "thresh_init", "thresh_refine", "force_loss", "ok_override")]

    def __init__(self, frame_id=0, last_keyframe_id=0, force=0, mapping_stopped=0, mapping_idle=1, mapping_queue_length=0, n_kfs_in_map=3, min_N_tracked_close=100,
                 thresh_N_nontracked_close=70, min_KF_interval=0, max_KF_interval=30, N_tracked_target=200, N_tracked_variance=50, th_depth=40.0, n_min_points=100,
                 thresh_init=10, thresh_refine=30, force_loss=0, ok_override=-1):
        super().__init__(frame_id, last_keyframe_id, force, mapping_stopped, mapping_idle, mapping_queue_length, n_kfs_in_map, min_N_tracked_close,
                         thresh_N_nontracked_close, min_KF_interval, max_KF_interval, N_tracked_target, N_tracked_variance, th_depth, n_min_points, thresh_init,
                         thresh_refine, force_loss, ok_override)


# the device outputs of hs_keyframe_create_device / hs_track_keyframe_device: (field, element dtype, count as a size name or a number, columns)
KEYFRAME_OUT_SPEC = (("result", "keyframe_result", 1), ("pose_view", "pose_view", 1), ("new_view", np.int32, "new_cap"), ("new_pos", np.float32, "new_cap3"),
                     ("entries", "lm_entry", "new_cap"), ("obs", "lm_obs", "new_cap"), ("obs_offsets", np.int64, "new_cap1"), ("desc_offsets", np.int64, "new_cap1"),
                     ("desc", np.uint8, "new_cap32"), ("lm_index", np.int32, "new_cap"))


class KeyFrameOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _, _ in KEYFRAME_OUT_SPEC] + [("lms", C.c_void_p), ("lms_cap", C.c_int32)]


class TrackOut(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k, _, _ in TRACK_OUT_HEAD] + [("local", LocalMapOut)] + [(k, C.c_void_p) for k, _, _ in TRACK_OUT_TAIL])


def track_out_dtype(kind):
    return {"pose_view": POSE_VIEW_DTYPE, "problem": POSE_PROBLEM_DTYPE, "lm": LM_DTYPE, "edge": POSE_EDGE_DTYPE, "result": POSE_RESULT_DTYPE,
            "track_result": TRACK_RESULT_DTYPE, "track_initial_result": TRACK_INITIAL_RESULT_DTYPE, "keyframe_result": KEYFRAME_RESULT_DTYPE, "lm_entry": LM_ENTRY_DTYPE, "lm_obs": LM_OBS_DTYPE}[kind] if isinstance(kind, str) else np.dtype(kind)


class FrameView(C.Structure):
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("mbf", C.c_float),
                ("sensor", C.c_int32), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("size_ref", C.c_float), ("n", C.c_int32),
                ("kps", C.c_void_p), ("desc", C.c_void_p), ("uR", C.c_void_p), ("kp_lm_obs", C.c_void_p)]


class VocabTree(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("levels", C.c_int32), ("child_begin", C.c_void_p), ("child_count", C.c_void_p),
                ("desc", C.c_void_p), ("word_id", C.c_void_p), ("weight", C.c_void_p), ("orig_id", C.c_void_p)]


class ProjParams(C.Structure):
    _fields_ = [("th", C.c_float), ("score_threshold", C.c_float), ("second_best_ratio", C.c_float),
                ("frac_smaller", C.c_float), ("frac_larger", C.c_float),
                ("use_distance", C.c_int32), ("use_stereo", C.c_int32), ("check_rotation", C.c_int32),
                ("use_prev_matched", C.c_int32), ("use_viewing_angle", C.c_int32), ("max_view_angle", C.c_float),
                ("use_reprojection", C.c_int32), ("reproj_threshold", C.c_float), ("sigma_ref", C.c_float), ("first_wins", C.c_int32),
                ("dist_is_invariance_range", C.c_int32)]

    def __init__(self, th=3.0, score_threshold=100.0, second_best_ratio=0.6, frac_smaller=0.5, frac_larger=1.5, use_distance=1, use_stereo=1,
                 check_rotation=0, use_prev_matched=1, use_viewing_angle=0, max_view_angle=1.047, use_reprojection=0, reproj_threshold=5.99,
                 sigma_ref=1.0, first_wins=0, dist_is_invariance_range=0):
        super().__init__(th, score_threshold, second_best_ratio, frac_smaller, frac_larger, use_distance, use_stereo, check_rotation,
                         use_prev_matched, use_viewing_angle, max_view_angle, use_reprojection, reproj_threshold, sigma_ref, first_wins, dist_is_invariance_range)


class HsError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("hyslam_amd: %s (status %d)" % (msg, status))
        self.status = status


# every symbol include/hyslam_amd.h declares (tests check the library exports all of them)
EXPORTS = [
    "hs_version", "hs_status_string", "hs_device_count", "hs_orb_default_params", "hs_orb_create", "hs_orb_destroy",
    "hs_orb_last_error", "hs_orb_get_levels", "hs_orb_get_device", "hs_orb_get_scale_factor", "hs_orb_get_scale_tables",
    "hs_orb_max_keypoints", "hs_orb_reserve", "hs_orb_extract", "hs_orb_extract_batch", "hs_orb_extract_batch_device",
    "hs_preprocess_size", "hs_preprocess_device", "hs_orb_extract_camera_batch", "hs_orb_submit_camera_batch",
    "hs_host_alloc", "hs_host_free", "hs_orb_submit_batch", "hs_orb_wait", "hs_orb_cancel", "hs_ticket_frames_copied",
    "hs_stereo_match", "hs_stereo_match_batch_device", "hs_stereo_frontend_batch_device", "hs_orb_set_lanes", "hs_orb_set_split", "hs_orb_synchronize",
    "hs_frame_grid", "hs_search_by_projection", "hs_search_by_projection_device", "hs_frame_publish", "hs_frame_find", "hs_frame_release", "hs_frame_info", "hs_frame_cache_clear", "hs_search_by_projection_frame", "hs_stereo_match_frames", "hs_search_by_projection_sim3", "hs_search_by_sim3", "hs_search_by_bow", "hs_search_by_bow_ex", "hs_search_by_bow_legacy", "hs_search_for_initialization",
    "hs_vocab_last_error", "hs_vocab_load", "hs_vocab_from_tree", "hs_vocab_save", "hs_vocab_destroy", "hs_vocab_get_tree", "hs_vocab_info",
    "hs_vocab_upload", "hs_vocab_dev_destroy", "hs_vocab_dev_groups", "hs_bow_transform_device", "hs_records_bow_match_device", "hs_bow_transform", "hs_hamming_knn2", "hs_hamming_knn2_device",
    "hs_record_bytes", "hs_record_offsets", "hs_records_knn2_device", "hs_landmark_best_descriptors", "hs_landmark_best_descriptors_device",
    "hs_landmark_update_entries", "hs_landmark_update_entries_device",
    "hs_kf_votes", "hs_kf_votes_device", "hs_kf_redundancy", "hs_kf_redundancy_device",
    "hs_local_keyframes", "hs_local_keyframes_device", "hs_local_points", "hs_local_points_device", "hs_local_points_work_bytes",
    "hs_landmark_gather_device", "hs_local_map_work_bytes", "hs_local_map_search_device",
    "hs_pose_optimize", "hs_pose_optimize_device", "hs_pose_work_bytes", "hs_pose_edges_device",
    "hs_pnp_plan", "hs_pnp_state_init", "hs_pnp_work_bytes", "hs_pnp_iterate", "hs_pnp_iterate_device",
    "hs_sim3_plan", "hs_sim3_state_init", "hs_sim3_work_bytes", "hs_sim3_iterate", "hs_sim3_iterate_device",
    "hs_monoinit_work_bytes", "hs_monoinit_check", "hs_monoinit_estimate", "hs_monoinit_estimate_device", "hs_debug_monoinit_layout",
    "hs_pose_views_device", "hs_search_by_projection_posed_device", "hs_local_map_search_posed_device", "hs_track_work_bytes", "hs_frame_associate_device",
    "hs_frame_views_device", "hs_track_discard_device", "hs_track_motion_model_device", "hs_track_local_map_device", "hs_track_frame_device",
    "hs_search_by_bow_kf_device", "hs_frame_associate_views_device", "hs_track_refkf_work_bytes",
    "hs_track_initial_work_bytes", "hs_track_reference_keyframe_device", "hs_track_initial_device", "hs_track_normal_device", "hs_device_alloc", "hs_device_free", "hs_device_copy",
    "hs_keyframe_work_bytes", "hs_keyframe_reference_device", "hs_keyframe_gate_device", "hs_keyframe_clean_device", "hs_keyframe_need_device",
    "hs_keyframe_create_device", "hs_keyframe_discard_device", "hs_track_keyframe_device",
    "hs_bow_vector", "hs_bow_vector_device", "hs_place_db_create", "hs_place_db_destroy", "hs_place_db_add", "hs_place_db_add_device", "hs_place_db_erase",
    "hs_place_db_clear", "hs_place_db_size", "hs_place_query_reloc", "hs_place_query_loop", "hs_place_query_reloc_device", "hs_place_query_loop_device",
    "hs_comm_available", "hs_comm_unavailable_reason", "hs_orb_borrowers", "hs_comm_get_unique_id", "hs_comm_create", "hs_comm_destroy", "hs_comm_rccl_ranks", "hs_comm_rccl_rank", "hs_comm_rccl_version", "hs_comm_world", "hs_comm_rank", "hs_comm_last_error", "hs_comm_allgather_records",
    "hs_orb_stage_launches", "hs_orb_profile_begin", "hs_orb_profile_pause", "hs_orb_profile_end", "hs_debug_stream_copy", "hs_debug_poison", "hs_debug_poison_violations", "hs_debug_poison_selftest",
    "hs_orb_debug_level", "hs_orb_set_debug", "hs_orb_debug_candidates", "hs_orb_debug_selected", "hs_orb_debug_quadtree_replay", "hs_debug_quadtree_level_fallbacks",
]

_lib = None

# source files each kernel family is compiled from: the committed rocprofv3 counter passes (profiles/*_{hbm_traffic,sq_counters}.json) are stamped
# with these digests and bench.py only replays a counter whose kernel sources are unchanged
KERNEL_SOURCES = {
    "k_fast_rows": ["kernels_fast.hip", "hs_fast.h", "hs_internal.h"],
    "k_resize": ["kernels_pyramid.hip", "hs_pyramid.h", "hs_internal.h"],
    "k_describe": ["kernels_describe.hip", "lean_sincos.h", "hs_internal.h"],
    "k_quadtree": ["kernels_quadtree.hip", "hs_internal.h"],
    "k_qt": ["kernels_quadtree.hip", "hs_internal.h"],
    "k_stereo": ["kernels_stereo.hip", "hs_internal.h"],
}


def source_digests():
    """{kernel-name prefix: sha256[:16] of the source files it is compiled from} (hyslam_amd/csrc travels with the repository snapshot)"""
    import hashlib
    out = {}
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    for k, files in KERNEL_SOURCES.items():
        h = hashlib.sha256()
        for f in files:
            try:
                h.update(open(os.path.join(src, f), "rb").read())
            except OSError:
                h.update(b"missing:" + f.encode())
        out[k] = h.hexdigest()[:16]
    return out



def lib():
    """Load the HIP library (once).  Raises if it is absent — build it with `python -c 'import __graft_entry__ as g; g.build()'`."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("hyslam_amd: %s not found; the HIP extension must be built (make -C hyslam_amd/csrc). "
                          "There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, f32, sz = C.c_void_p, C.c_int32, C.c_float, C.c_size_t
    L.hs_version.restype = C.c_char_p
    L.hs_status_string.restype = C.c_char_p
    L.hs_status_string.argtypes = [C.c_int]
    L.hs_device_count.argtypes = [C.POINTER(C.c_int)]
    L.hs_orb_default_params.argtypes = [C.POINTER(OrbParams)]
    L.hs_orb_default_params.restype = None
    L.hs_orb_create.argtypes = [C.POINTER(OrbParams), C.c_int, C.POINTER(vp)]
    L.hs_orb_destroy.argtypes = [vp]
    L.hs_orb_destroy.restype = None
    L.hs_orb_last_error.argtypes = [vp]
    L.hs_orb_last_error.restype = C.c_char_p
    L.hs_orb_get_levels.argtypes = [vp]
    L.hs_orb_get_device.argtypes = [vp]
    L.hs_orb_set_split.argtypes = [vp, C.c_int]
    L.hs_orb_get_scale_factor.argtypes = [vp]
    L.hs_orb_get_scale_factor.restype = f32
    L.hs_orb_get_scale_tables.argtypes = [vp, vp, vp, vp, vp, vp]
    L.hs_orb_max_keypoints.argtypes = [vp]
    L.hs_orb_reserve.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.hs_orb_extract.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp]
    L.hs_orb_extract_batch.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp]
    L.hs_orb_extract_batch_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, sz, sz, vp, vp, vp, C.c_int, vp]
    L.hs_preprocess_size.argtypes = [C.c_int, C.c_int, f32, vp, vp]
    L.hs_preprocess_size.restype = None
    L.hs_preprocess_device.argtypes = [vp, vp, C.c_int, C.c_int, sz, sz, C.c_int, C.POINTER(PreprocessParams), vp, sz, sz, vp]
    L.hs_orb_extract_camera_batch.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, sz, C.POINTER(PreprocessParams), vp, vp, C.c_int, vp, vp]
    L.hs_orb_submit_camera_batch.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, sz, C.POINTER(PreprocessParams), vp, C.POINTER(i32)]
    L.hs_stereo_match.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.POINTER(StereoParams), vp, vp]
    L.hs_stereo_match_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(StereoParams), vp, vp, vp]
    L.hs_stereo_frontend_batch_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, sz, sz,
                                                  vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(StereoParams), vp, vp, vp]
    L.hs_orb_set_lanes.argtypes = [vp, C.c_int]
    L.hs_orb_synchronize.argtypes = [vp, vp]
    L.hs_frame_grid.argtypes = [vp, C.POINTER(FrameView), vp]
    L.hs_search_by_projection.argtypes = [vp, C.POINTER(FrameView), vp, C.c_int, C.POINTER(ProjParams), vp, vp, vp]
    L.hs_search_by_projection_device.argtypes = [vp, C.POINTER(FrameView), vp, C.c_int, C.POINTER(ProjParams), vp, vp, vp, vp]
    u64 = C.c_uint64
    L.hs_frame_publish.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(u64)]
    L.hs_frame_find.argtypes = [C.c_int, vp, C.c_int, C.POINTER(u64)]
    L.hs_frame_release.argtypes = [C.c_int, u64]
    L.hs_frame_info.argtypes = [C.c_int, u64, vp]
    L.hs_frame_cache_clear.argtypes = [C.c_int]
    L.hs_search_by_projection_frame.argtypes = [vp, u64, C.POINTER(FrameView), vp, C.c_int, C.POINTER(ProjParams), vp, vp, vp]
    L.hs_stereo_match_frames.argtypes = [vp, u64, u64, C.POINTER(StereoParams), vp, vp]
    L.hs_search_by_projection_sim3.argtypes = [vp, C.POINTER(FrameView), vp, vp, C.c_int, C.c_int, f32, vp, vp, vp]
    L.hs_search_by_sim3.argtypes = [vp, C.POINTER(FrameView), vp, C.POINTER(FrameView), vp, f32, vp, vp, f32, f32, vp, vp]
    L.hs_search_by_bow.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_int,
                                   vp, f32, f32, C.c_int, vp, vp]
    L.hs_search_by_bow_ex.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_int,
                                      vp, vp, vp, f32, f32, f32, f32, C.c_int, vp, vp]
    L.hs_search_by_bow_legacy.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_int,
                                          vp, vp, f32, f32, C.c_int, vp, vp]
    L.hs_search_for_initialization.argtypes = [vp, vp, vp, C.c_int, C.POINTER(FrameView), vp, C.c_int, f32, f32, vp, vp]
    L.hs_vocab_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.hs_vocab_from_tree.argtypes = [C.POINTER(VocabTree), C.c_int, C.POINTER(vp)]
    L.hs_vocab_save.argtypes = [vp, C.c_char_p]
    L.hs_vocab_destroy.argtypes = [vp]
    L.hs_vocab_destroy.restype = None
    L.hs_vocab_get_tree.argtypes = [vp, C.POINTER(VocabTree)]
    L.hs_vocab_info.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.hs_vocab_upload.argtypes = [vp, C.POINTER(VocabTree), C.c_int, C.POINTER(vp)]
    L.hs_vocab_dev_destroy.argtypes = [vp]
    L.hs_vocab_dev_destroy.restype = None
    L.hs_vocab_dev_groups.argtypes = [vp]
    L.hs_bow_transform_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]
    L.hs_records_bow_match_device.argtypes = [vp, vp, vp, sz, C.c_int, C.c_int, C.c_int, f32, f32, C.c_int, vp, vp, vp]
    L.hs_bow_transform.argtypes = [vp, C.POINTER(VocabTree), vp, C.c_int, C.c_int, vp, vp, vp]
    L.hs_hamming_knn2.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp, vp]
    L.hs_hamming_knn2_device.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    L.hs_record_bytes.argtypes = [C.c_int]
    L.hs_record_bytes.restype = sz
    L.hs_record_offsets.argtypes = [C.c_int, vp, vp, vp]
    L.hs_record_offsets.restype = None
    L.hs_records_knn2_device.argtypes = [vp, vp, sz, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.hs_landmark_best_descriptors.argtypes = [vp, vp, vp, C.c_int, vp, vp]
    L.hs_landmark_best_descriptors_device.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp]
    L.hs_landmark_update_entries.argtypes = [vp, vp, C.c_int] + [vp] * 13
    L.hs_landmark_update_entries_device.argtypes = [vp, vp, C.c_int] + [vp] * 15 + [C.c_int, vp]
    L.hs_kf_votes.argtypes = [vp, C.POINTER(KfTable), C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp]
    L.hs_kf_votes_device.argtypes = L.hs_kf_votes.argtypes + [vp]
    L.hs_kf_redundancy.argtypes = [vp, C.POINTER(KfTable), C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, f32, vp, vp, vp]
    L.hs_kf_redundancy_device.argtypes = L.hs_kf_redundancy.argtypes + [vp]
    L.hs_local_keyframes.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp]
    L.hs_local_keyframes_device.argtypes = L.hs_local_keyframes.argtypes + [vp]
    L.hs_local_points.argtypes = [vp, C.POINTER(KfTable), vp, vp, C.c_int, vp, vp, C.c_int, vp]
    L.hs_local_points_device.argtypes = L.hs_local_points.argtypes + [vp, vp]
    L.hs_landmark_gather_device.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, vp, vp]
    L.hs_local_map_search_device.argtypes = [vp, C.POINTER(KfTable), vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(FrameView), vp,
                                             C.POINTER(ProjParams), C.c_int, C.POINTER(LocalMapOut), vp, vp]
    for f in (L.hs_local_points_work_bytes, L.hs_local_map_work_bytes):
        f.argtypes, f.restype = [C.c_int], C.c_size_t
    L.hs_pose_optimize.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    L.hs_pose_optimize_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]
    L.hs_pose_work_bytes.argtypes, L.hs_pose_work_bytes.restype = [C.c_int, C.c_int64], C.c_size_t
    L.hs_pose_edges_device.argtypes = [vp, C.POINTER(FrameView), vp, C.c_int, vp, f32, vp, C.c_int, vp, vp, vp]
    L.hs_pnp_plan.argtypes = [C.c_int, C.POINTER(PnpParams), C.POINTER(PnpPlan)]
    L.hs_pnp_state_init.argtypes, L.hs_pnp_state_init.restype = [C.POINTER(PnpState)], None
    L.hs_pnp_work_bytes.argtypes, L.hs_pnp_work_bytes.restype = [C.c_int, C.c_int64, C.c_int], C.c_size_t
    L.hs_pnp_iterate.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    L.hs_pnp_iterate_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.hs_sim3_plan.argtypes = [C.c_int, C.POINTER(Sim3Params), C.POINTER(Sim3Plan)]
    L.hs_sim3_state_init.argtypes, L.hs_sim3_state_init.restype = [C.POINTER(Sim3State)], None
    L.hs_sim3_work_bytes.argtypes, L.hs_sim3_work_bytes.restype = [C.c_int, C.c_int64, C.c_int], C.c_size_t
    L.hs_sim3_iterate.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    L.hs_sim3_iterate_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.hs_monoinit_work_bytes.argtypes, L.hs_monoinit_work_bytes.restype = [C.c_int, C.c_int64, C.c_int], C.c_size_t
    L.hs_monoinit_check.argtypes, L.hs_monoinit_check.restype = [C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp], C.c_char_p
    L.hs_debug_monoinit_layout.argtypes = [C.c_int]
    L.hs_monoinit_estimate.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]
    L.hs_monoinit_estimate_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.hs_pose_views_device.argtypes = [vp, vp, vp, vp]
    L.hs_search_by_projection_posed_device.argtypes = [vp, C.POINTER(FrameView), vp, vp, C.c_int, C.POINTER(ProjParams), vp, vp, vp, vp]
    L.hs_local_map_search_posed_device.argtypes = [vp, C.POINTER(KfTable), vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(FrameView), vp, vp,
                                                   C.POINTER(ProjParams), C.c_int, C.POINTER(LocalMapOut), vp, vp]
    L.hs_track_work_bytes.argtypes, L.hs_track_work_bytes.restype = [C.c_int] * 4, C.c_size_t
    L.hs_frame_associate_device.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp]
    L.hs_frame_views_device.argtypes = [vp, C.c_int, vp, vp, vp, C.POINTER(KfTable), C.c_int, vp, vp]
    L.hs_track_discard_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, C.POINTER(KfTable), C.c_int, vp, vp, vp, vp, vp]
    tail = [C.POINTER(TrackParams), C.POINTER(TrackState), C.POINTER(TrackOut), vp, vp]
    L.hs_track_motion_model_device.argtypes = [vp, C.POINTER(FrameView), vp, vp, vp, C.c_int, C.POINTER(KfTable), vp] + tail
    L.hs_track_local_map_device.argtypes = [vp, C.POINTER(FrameView), vp, C.POINTER(KfTable), vp, vp, C.c_int, vp, C.c_int] + tail
    L.hs_track_frame_device.argtypes = [vp, C.POINTER(FrameView), vp, vp, vp, C.c_int, C.POINTER(KfTable), vp, vp, C.c_int, vp, C.c_int] + tail
    L.hs_search_by_bow_kf_device.argtypes = [vp, C.POINTER(KfFeatures), vp, C.POINTER(KfTable), vp, vp, vp, vp, C.c_int, f32, f32, vp, C.c_int, vp, vp, vp, vp, vp]
    L.hs_frame_associate_views_device.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.hs_track_refkf_work_bytes.argtypes, L.hs_track_refkf_work_bytes.restype = [C.c_int] * 3, C.c_size_t
    L.hs_track_initial_work_bytes.argtypes, L.hs_track_initial_work_bytes.restype = [C.c_int] * 5, C.c_size_t
    refkf = [vp, C.POINTER(KfFeatures), vp, C.c_int, vp, vp]                # vocab, K, d_kf_slot, kf_cap, d_Tcw_last, d_Tcw_entry
    itail = [C.POINTER(TrackParams), C.POINTER(TrackRefkfParams), C.POINTER(TrackState)]
    L.hs_track_reference_keyframe_device.argtypes = [vp, C.POINTER(FrameView)] + refkf + [vp, C.POINTER(KfTable), vp] + itail + [C.POINTER(TrackInitialOut), vp, vp]
    motion = [vp, C.POINTER(FrameView), C.c_int, vp, vp, vp, C.c_int]       # h, F, velocity_valid, d_Tcw_pred, d_last_kps, d_last_kp_lm, n_last
    L.hs_track_initial_device.argtypes = motion + refkf + [C.POINTER(KfTable), vp] + itail + [C.POINTER(TrackOut), C.POINTER(TrackInitialOut), vp, vp]
    L.hs_track_normal_device.argtypes = (motion + refkf + [C.POINTER(KfTable), vp, vp, C.c_int, vp, C.c_int] + itail +
                                         [C.POINTER(TrackOut), C.POINTER(TrackInitialOut), vp, vp])
    L.hs_keyframe_work_bytes.argtypes, L.hs_keyframe_work_bytes.restype = [C.c_int] * 3, C.c_size_t
    kst, kpr = C.POINTER(TrackState), C.POINTER(KeyFrameParams)
    L.hs_keyframe_reference_device.argtypes = [vp, C.c_int, kst, C.POINTER(KfTable), vp, vp, vp, vp]
    L.hs_keyframe_gate_device.argtypes = [vp, vp, kpr, vp, vp]
    L.hs_keyframe_clean_device.argtypes = [vp, C.c_int, kst, C.POINTER(KfTable), vp, vp]
    L.hs_keyframe_need_device.argtypes = [vp, C.c_int, C.c_int, vp, kst, C.POINTER(KfTable), C.POINTER(KfFeatures), vp, vp, kpr, vp, vp]
    L.hs_keyframe_create_device.argtypes = [vp, C.POINTER(FrameView), vp, vp, kst, C.POINTER(KfTable), kpr, C.c_int, C.POINTER(KeyFrameOut), vp, vp]
    L.hs_keyframe_discard_device.argtypes = [vp, C.c_int, kst, vp, vp]
    L.hs_track_keyframe_device.argtypes = [vp, C.POINTER(FrameView), vp, vp, C.POINTER(KfTable), C.POINTER(KfFeatures), vp, kpr, kst, vp, C.c_int,
                                           C.POINTER(KeyFrameOut), vp, vp]
    L.hs_device_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    L.hs_device_free.argtypes = [vp, vp]
    L.hs_device_copy.argtypes = [vp, vp, vp, sz, C.c_int, vp]
    L.hs_bow_vector.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp]
    L.hs_bow_vector_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]
    L.hs_place_db_create.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.hs_place_db_destroy.argtypes = [vp]
    L.hs_place_db_destroy.restype = None
    L.hs_place_db_add.argtypes = [vp, C.c_uint64, vp, vp, C.c_int, vp]
    L.hs_place_db_add_device.argtypes = [vp, C.c_uint64, vp, vp, vp, C.c_int, vp, vp]
    L.hs_place_db_erase.argtypes = [vp, i32]
    L.hs_place_db_clear.argtypes = [vp]
    L.hs_place_db_size.argtypes = [vp, vp, vp]
    L.hs_place_query_reloc.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp]
    L.hs_place_query_loop.argtypes = [vp, vp, vp, C.c_int, vp, f32, vp, vp, C.c_int, vp, vp, vp, vp, vp]
    L.hs_place_query_reloc_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.hs_place_query_loop_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, f32, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.hs_host_alloc.argtypes = [sz, C.POINTER(vp)]
    L.hs_host_free.argtypes = [vp]
    L.hs_host_free.restype = None
    L.hs_orb_submit_batch.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.POINTER(i32)]
    L.hs_orb_wait.argtypes = [vp, i32, vp, vp, vp, C.c_int, vp, vp]
    L.hs_orb_cancel.argtypes = [vp, i32]
    L.hs_ticket_frames_copied.argtypes = [vp, i32]
    L.hs_comm_get_unique_id.argtypes = [vp]
    L.hs_vocab_last_error.argtypes = []
    L.hs_vocab_last_error.restype = C.c_char_p
    L.hs_comm_available.argtypes = []
    L.hs_comm_unavailable_reason.argtypes = []
    L.hs_comm_unavailable_reason.restype = C.c_char_p
    L.hs_orb_borrowers.argtypes = [vp]
    L.hs_comm_create.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.hs_comm_destroy.argtypes = [vp]
    L.hs_comm_destroy.restype = None
    L.hs_comm_world.argtypes = [vp]
    L.hs_comm_rank.argtypes = [vp]
    L.hs_comm_last_error.argtypes = [vp]
    L.hs_comm_last_error.restype = C.c_char_p
    L.hs_comm_allgather_records.argtypes = [vp, vp, vp, sz, vp]
    L.hs_debug_stream_copy.argtypes = [vp, vp, vp, sz, C.c_int, vp]
    L.hs_debug_poison.argtypes = [C.c_int]
    L.hs_debug_poison_violations.restype = C.c_longlong
    L.hs_debug_poison_violations.argtypes = []
    L.hs_debug_poison_selftest.argtypes = [vp, vp]
    L.hs_orb_stage_launches.argtypes = [vp, C.c_int]
    L.hs_orb_profile_begin.argtypes = [vp]
    L.hs_orb_profile_pause.argtypes = [vp]
    L.hs_orb_profile_end.argtypes = [vp, vp, vp]
    L.hs_orb_debug_level.argtypes = [vp, C.c_int, C.c_int, vp, sz, vp, vp]
    L.hs_orb_set_debug.argtypes = [vp, C.c_int]
    L.hs_orb_debug_candidates.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp]
    L.hs_orb_debug_selected.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp]
    L.hs_debug_quadtree_level_fallbacks.restype = C.c_longlong
    L.hs_debug_quadtree_level_fallbacks.argtypes = [C.c_int]
    L.hs_orb_debug_quadtree_replay.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    _lib = L
    return L


def check(handle, status):
    if status != HS_OK:
        L = lib()
        msg = L.hs_status_string(status).decode()
        if handle:
            detail = L.hs_orb_last_error(handle).decode()
            if detail:
                msg += ": " + detail
        raise HsError(status, msg)
