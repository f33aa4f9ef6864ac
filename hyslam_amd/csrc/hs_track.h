// hs_track.h — frame tracking on resident tables (TrackMotionModel::track, TrackLocalMap::track): launchers of kernels_track.hip for the entry
// points in hs_track.hip (include/hyslam_amd.h).  All asynchronous on `s`; every pointer is device memory unless said otherwise.
#pragma once
#include "hs_internal.h"

#define HS_TRACK_BLOCK 256         // threads per workgroup of the per-view / per-op kernels

inline bool state_ok(const hs_track_state* s) { return s && s->kp_lm && s->kp_outl && s->n_matches && s->kp_lm_obs; }
inline bool feats_ok(const hs_kf_features* K) { return K && K->n_kf >= 0 && K->kf_off && K->kps && K->desc && K->node && K->kp_lm; }
inline bool track_out_ok(const hs_track_out* o)
{
    return o && o->pose_view && o->problem && o->last_lms && o->narrow_idx && o->narrow_dist && o->narrow_n && o->wide_idx && o->wide_dist && o->wide_n && o->op_view &&
           o->edges_motion && o->outlier_motion && o->n_edges_motion && o->pose_motion && o->edges_local && o->outlier_local && o->n_edges_local && o->pose_local &&
           o->result && !((uintptr_t)o->last_lms & 15) && !((uintptr_t)o->edges_motion & 15) && !((uintptr_t)o->edges_local & 15);
}

// d_problem (may be nullptr): the optimiser's hs_pose_problem = the pose with F's camera (F: host struct, only fx .. mbf are read)
void hs_launch_pose_view(const float* d_Tcw, hs_pose_view* d_out, hs_pose_problem* d_problem, const hs_frame_view* F, hipStream_t s);
void hs_launch_frame_associate(int n, int L, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, int n_ops, const int32_t* d_op_view, const int32_t* d_op_lm,
                               const HsAssocWork& w, hipStream_t s);
void hs_launch_frame_views(int n, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, const hs_kf_table& T, int drop_bad, int32_t* d_kp_lm_obs, hipStream_t s);
void hs_launch_track_discard(int mode, const hs_pose_edge* d_edges, const int32_t* d_n_edges, int edge_cap, const uint8_t* d_outlier, const hs_pose_result* d_result,
                             const hs_kf_table& T, int sensor, int n, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, int32_t* d_counts, hipStream_t s);
void hs_launch_last_gather(const hs_landmark* d_lms, int L, const int32_t* d_last_kp_lm, const hs_keypoint* d_last_kps, int n_last, hs_landmark* d_out, hipStream_t s);
void hs_launch_track_clear(int n, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, int32_t* d_kp_lm_obs, hipStream_t s);
void hs_launch_track_select(int n_last, const int32_t* d_narrow_idx, const int32_t* d_narrow_n, const int32_t* d_wide_idx, const int32_t* d_wide_n, int n_min_matches,
                            int32_t* d_op_view, hs_track_result* d_result, hipStream_t s);
void hs_launch_track_gate(const hs_track_result* d_result, int32_t* d_n_edges /*[2]: [1] = failed ? 0 : [0]*/, hipStream_t s);

// ---- SearchByBoW(KeyFrame*, Frame&) and associateLandMarks in view order (kernels_track_refkf.hip; entry points in hs_track_refkf.hip)
void hs_launch_search_by_bow_kf(const hs_kf_features& K, const int32_t* d_kf_slot, const hs_kf_table& T, const hs_keypoint* d_kps, const uint8_t* d_desc,
                                const int32_t* d_node, const float* d_weight /*may be nullptr*/, int n, float th_low, float nnratio, int32_t* d_match_kf, int kf_cap,
                                int32_t* d_op_view, int32_t* d_op_lm, int32_t* d_n_matches, hipStream_t s);
void hs_launch_frame_associate_views(int n, int L, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, const int32_t* d_op_view, const int32_t* d_op_lm,
                                     const HsVassocWork& w, hipStream_t s);

// ---- the gates of initialPoseEstimation (kernels_track_initial.hip; entry points in hs_track_initial.hip).  d_motion: the motion stage's result, or
// nullptr for a stage that is not predicated on one.  Every kernel reads its gate from *d_result, where hs_launch_init_gate left it.
void hs_launch_init_gate(int n, const hs_track_result* d_motion, const hs_track_refkf_params& rp, const int32_t* d_op_view, const int32_t* d_op_lm,
                         int32_t* d_op_view_run /*[n]: the op, or -1 unless the stage runs*/, int32_t* d_op_lm_run, hs_track_initial_result* d_result /*n_bow holds the search's count*/, hipStream_t s);
void hs_launch_init_edges_gate(const hs_track_initial_result* d_result, int32_t* d_n_edges /*[2]: [1] = OK ? [0] : 0*/, hipStream_t s);
void hs_launch_init_finish(const hs_track_result* d_motion, int thresh_init, const hs_pose_result* d_pose, const float* d_Tcw_entry, float* d_Tcw_init /*[16]*/,
                           hs_track_initial_result* d_result /*n_matches_map_refkf holds the discard's count*/, hipStream_t s);
void hs_launch_frame_result(const hs_track_result* d_motion, const hs_track_initial_result* d_init, const int32_t* d_n_inliers, hs_track_result* d_out, hipStream_t s);

// ---- reference key frame, key-frame decision, stereo landmark creation (kernels_keyframe.hip; entry points in hs_keyframe.hip).  Every kernel reads
// its gate (ok / insert / n_processed) from *d_result, where an earlier launch left it.
void hs_launch_kfd_ref_begin(int n, int64_t* d_q_off /*[2] = {0, n}*/, hipStream_t s);
void hs_launch_kfd_ref_update(const int32_t* d_max_slot, int32_t* d_ref_slot, hs_keyframe_result* d_result, hipStream_t s);
void hs_launch_kfd_gate(const hs_track_result* d_track_result, const hs_keyframe_params& p, hs_keyframe_result* d_result, hipStream_t s);
void hs_launch_kfd_clean(int n, const hs_track_state& st, const hs_kf_table& T, hs_keyframe_result* d_result, hipStream_t s);
void hs_launch_kfd_need(int n, int sensor, const float* d_depth, const hs_track_state& st, const hs_kf_table& T, const hs_kf_features& K, const int32_t* d_ref_slot,
                        const hs_track_result* d_track_result, const hs_keyframe_params& p, hs_keyframe_result* d_result, hipStream_t s);
void hs_launch_kfd_create(const hs_frame_view& F, const float* d_depth, const hs_track_state& st, const hs_kf_table& T, const hs_keyframe_params& p, int new_cap,
                          const hs_keyframe_out& out, unsigned long long* d_keys /*[n]*/, hipStream_t s);
void hs_launch_kfd_discard(int n, const hs_track_state& st, const hs_keyframe_result* d_result, hipStream_t s);
