// hs_track.h — the resident chain (frame tracking on resident tables and the stages around it): the predicate of every `_device` entry point that is a
// stage of a chain, the enqueues and plans the chains share, and the launchers of kernels_track*.hip / kernels_keyframe.hip for the entry points in
// hs_track*.hip and hs_keyframe.hip (include/hyslam_amd.h).  All asynchronous on `s`; every pointer is device memory unless said otherwise.
#pragma once
#include "hs_poseopt.h"
#include <initializer_list>

#define HS_TRACK_BLOCK 256         // threads per workgroup of the per-view / per-op kernels

inline bool state_ok(const hs_track_state* s) { return s && s->kp_lm && s->kp_outl && s->n_matches && s->kp_lm_obs; }
inline bool feats_ok(const hs_kf_features* K) { return K && K->n_kf >= 0 && K->kf_off && K->kps && K->desc && K->node && K->kp_lm; }
inline bool track_out_ok(const hs_track_out* o)
{
    return o && o->pose_view && o->problem && o->last_lms && o->narrow_idx && o->narrow_dist && o->narrow_n && o->wide_idx && o->wide_dist && o->wide_n && o->op_view &&
           o->edges_motion && o->outlier_motion && o->n_edges_motion && o->pose_motion && o->edges_local && o->outlier_local && o->n_edges_local && o->pose_local &&
           o->result && !((uintptr_t)o->last_lms & 15) && !((uintptr_t)o->edges_motion & 15) && !((uintptr_t)o->edges_local & 15);
}
inline const char* hs_first(std::initializer_list<const char*> whys) { for (const char* w : whys) if (w) return w; return nullptr; }

// ---- what every stage of the resident chain refuses: the predicate of its `_device` entry point (hs_device_call, hs_internal.h), which is what the
// entry point refuses when called directly and what a composite calls on the expressions it hands the stage.  Pure host code: the by-value arguments
// and the host structs, nothing from device memory, no handle (hs_bow_transform_why, over the opaque hs_vocab_dev, is in kernels_bow.hip).
inline const char* hs_pose_views_why(const float* d_Tcw, const hs_pose_view* d_out) { return hs_bad(!d_Tcw || !d_out); }
inline const char* hs_frame_associate_why(int n, int L, const int32_t* d_kp_lm, const uint8_t* d_kp_outl, const int32_t* d_n_matches, int n_ops, const int32_t* d_op_view,
                                          const int32_t* d_op_lm, const void* d_work)
{
    return hs_bad(n < 0 || L < 0 || n_ops < 0 || !d_n_matches || !d_work || (n > 0 && (!d_kp_lm || !d_kp_outl)) || (n_ops > 0 && (!d_op_view || !d_op_lm)));
}
inline const char* hs_frame_views_why(int n, const int32_t* d_kp_lm, const uint8_t* d_kp_outl, const int32_t* d_n_matches, const hs_kf_table* T, int drop_bad,
                                      const int32_t* d_kp_lm_obs)
{
    return hs_bad(n < 0 || n > 65535 || !T || T->L < 0 || (n > 0 && (!d_kp_lm || !d_kp_lm_obs)) || (T->L > 0 && !T->lm_nobs) ||
                  (drop_bad && (!d_kp_outl || !d_n_matches || (T->L > 0 && !T->lm_bad))));
}
inline const char* hs_track_discard_why(int mode, const hs_pose_edge* d_edges, const int32_t* d_n_edges, int edge_cap, const uint8_t* d_outlier, const hs_pose_result* d_result,
                                        const hs_kf_table* T, const int32_t* d_kp_lm, const uint8_t* d_kp_outl, const int32_t* d_n_matches, const int32_t* d_counts)
{
    return hs_bad((mode != HS_TRACK_MOTION && mode != HS_TRACK_LOCAL) || !d_n_edges || edge_cap < 0 || !d_result || !T || T->L < 0 || (T->L > 0 && !T->lm_nobs) ||
                  !d_n_matches || !d_counts || (edge_cap > 0 && (!d_edges || !d_outlier || !d_kp_lm || !d_kp_outl)));
}
inline const char* hs_search_by_bow_kf_why(const hs_kf_features* K, const int32_t* d_kf_slot, const hs_kf_table* T, const hs_keypoint* d_kps, const uint8_t* d_desc,
                                           const int32_t* d_node, int n, const int32_t* d_match_kf, int kf_cap, const int32_t* d_op_view, const int32_t* d_op_lm,
                                           const int32_t* d_n_matches)
{
    return hs_bad(!feats_ok(K) || !d_kf_slot || !T || T->L < 0 || (T->L > 0 && !T->lm_bad) || n < 1 || n > 65535 || !d_kps || !d_desc || !d_node || kf_cap < 1 ||
                  !d_match_kf || !d_op_view || !d_op_lm || !d_n_matches);
}
inline const char* hs_frame_associate_views_why(int n, int L, const int32_t* d_kp_lm, const uint8_t* d_kp_outl, const int32_t* d_n_matches, const int32_t* d_op_view,
                                                const int32_t* d_op_lm, const void* d_work)
{
    return hs_bad(n < 0 || L < 0 || !d_n_matches || !d_work || (n > 0 && (!d_kp_lm || !d_kp_outl || !d_op_view || !d_op_lm)));
}
inline const char* hs_search_by_projection_why(const hs_frame_view* F, const hs_landmark* d_lms, int L, const hs_proj_params* pp, const int32_t* d_match_idx,
                                               const float* d_match_dist, const int32_t* d_n_matches)
{
    return hs_bad(!F || !pp || L < 1 || !d_lms || !d_match_idx || !d_match_dist || !d_n_matches || F->n < 1 || F->n > 65535 || !F->kps || !F->desc ||
                  (pp->use_stereo && F->sensor != 0 && !F->uR));
}
inline const char* hs_pose_edges_why(const hs_frame_view* F, const hs_landmark* d_lms, int L, const int32_t* d_kp_lm, const hs_pose_edge* d_edges, int cap,
                                     const int32_t* d_n_edges)
{
    return hs_bad(!F || F->n < 0 || L < 0 || cap < 0 || !d_n_edges || (cap > 0 && !d_edges) || (F->n > 0 && (!F->kps || !d_kp_lm)) || (L > 0 && !d_lms));
}
inline const char* hs_pose_optimize_why(int Q, const hs_pose_problem* d_problems, const int64_t* d_edge_offsets, const int32_t* d_n_edges, int edge_cap,
                                        const hs_pose_edge* d_edges, const hs_pose_result* d_results)
{
    return Q < 0 || (Q > 0 && (!d_problems || !d_results)) || (d_edge_offsets != nullptr) == (d_n_edges != nullptr) || (d_n_edges && (Q != 1 || edge_cap < 0)) ||
           ((uintptr_t)d_edges & 15) ? "bad argument (exactly one of d_edge_offsets and d_n_edges; d_n_edges needs Q == 1; d_edges is 16-byte aligned)" : nullptr;
}
inline const char* hs_kf_votes_why(const hs_kf_table* T, int Q, const int64_t* d_q_offsets, const int32_t* d_weights, const int32_t* d_max_slot, const int32_t* d_max_count,
                                   const int32_t* d_ordered_slot, const int32_t* d_ordered_weight, int cap, const int32_t* d_n_ordered)
{
    if (!T || Q < 0 || cap < 0 || T->L < 0 || T->n_kf < 0) return "bad argument";
    if (Q == 0) return nullptr;                                      // nothing to vote on: the pointers are not looked at
    if (!T->lm_obs_offsets || !d_q_offsets || !d_max_slot || !d_max_count || !d_n_ordered || (cap > 0 && (!d_ordered_slot || !d_ordered_weight)) ||
        (T->n_kf > 0 && (!T->kf_bad || !T->kf_id)) || (T->L > 0 && !T->lm_bad))
        return "bad argument";
    return T->n_kf > HS_KF_LDS_SLOTS && !d_weights ? "beyond HS_KF_LDS_SLOTS key frames the weights rows are the counters: d_weights is required" : nullptr;
}
inline const char* hs_local_keyframes_why(int n_kf, const int32_t* d_weights, const uint8_t* d_kf_bad, const int32_t* d_neigh, int neigh_cap, const int32_t* d_parent,
                                          const uint8_t* d_local, const int32_t* d_n_local)
{
    return hs_bad(n_kf < 0 || neigh_cap < 0 || !d_n_local || (n_kf > 0 && (!d_weights || !d_kf_bad || !d_parent || !d_local || (neigh_cap > 0 && !d_neigh))));
}
inline const char* hs_local_points_why(const hs_kf_table* T, const uint8_t* d_local, const int32_t* d_frame_lm, int n_assoc, const uint8_t* d_frame_remove,
                                       const int32_t* d_sel, int cap, const int32_t* d_n_sel, const void* d_work)
{
    return hs_bad(!T || T->L < 0 || T->n_kf < 0 || n_assoc < 0 || cap < 0 || !d_n_sel || !d_work || (cap > 0 && !d_sel) || (n_assoc > 0 && (!d_frame_lm || !d_frame_remove)) ||
                  (T->L > 0 && (!T->lm_obs_offsets || !T->lm_bad)) || (T->n_kf > 0 && !d_local));
}
inline const char* hs_landmark_gather_why(const hs_landmark* d_lms, int L, const int32_t* d_sel, const int32_t* d_n_sel, int cap, const hs_landmark* d_out)
{
    return L < 0 || cap < 0 || !d_n_sel || (cap > 0 && (!d_sel || !d_out)) || (L > 0 && !d_lms) || ((uintptr_t)d_lms & 15) || ((uintptr_t)d_out & 15)
               ? "bad argument (d_lms and d_out are 16-byte aligned)" : nullptr;
}
// the stages after the two track functions (hs_keyframe.hip)
inline bool kf_n_ok(int n) { return n >= 1 && n <= 65535; }
inline bool kf_table_ok(const hs_kf_table* T) { return T && T->L >= 0 && (T->L == 0 || (T->lm_nobs && T->lm_bad)); }
inline bool keyframe_out_ok(const hs_keyframe_out* o, int new_cap)
{
    return o && new_cap >= 0 && o->result && o->pose_view && o->obs_offsets && o->desc_offsets && (!o->lms || (o->lms_cap >= 0 && !((uintptr_t)o->lms & 15))) &&
           (new_cap == 0 || (o->new_view && o->new_pos && o->entries && o->obs && o->desc && o->lm_index));
}
inline const char* hs_keyframe_gate_why(const hs_track_result* d_track_result, const hs_keyframe_params* prm, const hs_keyframe_result* d_result)
{
    return hs_bad(!prm || !d_result || (prm->ok_override < 0 && !d_track_result));
}
inline const char* hs_keyframe_clean_why(int n, const hs_track_state* st, const hs_kf_table* T, const hs_keyframe_result* d_result)
{
    return hs_bad(!kf_n_ok(n) || !state_ok(st) || !kf_table_ok(T) || !d_result);
}
inline const char* hs_keyframe_need_why(int n, int sensor, const float* d_depth, const hs_track_state* st, const hs_kf_table* T, const hs_kf_features* K,
                                        const int32_t* d_ref_slot, const hs_keyframe_params* prm, const hs_keyframe_result* d_result)
{
    return hs_bad(!kf_n_ok(n) || (sensor != 0 && !d_depth) || !state_ok(st) || !kf_table_ok(T) || !K || K->n_kf < 0 || (K->n_kf > 0 && (!K->kf_off || !K->kp_lm)) ||
                  !d_ref_slot || !prm || !d_result);
}
inline const char* hs_keyframe_discard_why(int n, const hs_track_state* st, const hs_keyframe_result* d_result) { return hs_bad(!kf_n_ok(n) || !state_ok(st) || !d_result); }
const char* hs_bow_transform_why(const hs_vocab_dev* v, int device /*the handle's*/, const uint8_t* d_desc, int n_max, const int32_t* d_word, const float* d_weight,
                                 const int32_t* d_node);

// ---- the enqueues that are more than one launcher of this header, hs_poseopt.h or hs_internal.h: no check, no hipSetDevice, no hipGetLastError
void hs_kf_votes_enqueue(const hs_kf_table* T, int Q, const int64_t* d_q_offsets, const int32_t* d_q_lm, const int64_t* d_q_self_id, int count_bad_kf, int th,
                         int32_t* d_weights, int32_t* d_max_slot, int32_t* d_max_count, int32_t* d_ordered_slot, int32_t* d_ordered_weight, int cap, int32_t* d_n_ordered,
                         hipStream_t s);                             // hs_kfgraph.hip
void hs_bow_transform_enqueue(const hs_vocab_dev* v, const uint8_t* d_desc, const int32_t* d_n, int n_max, int32_t* d_word, float* d_weight, int32_t* d_node,
                              hipStream_t s);                        // kernels_bow.hip
// d_pose (may be nullptr): the pose comes from it, not from F.  The grid lists are claimed from the handle's scratch: HS_ERR_HIP where a regrow fails
int hs_search_by_projection_enqueue(hs_orb* h, const hs_frame_view* F, const hs_pose_view* d_pose, const hs_landmark* d_lms, int L, const hs_proj_params* pp,
                                    int32_t* d_match_idx, float* d_match_dist, int32_t* d_n_matches, hipStream_t s);                         // hs_api.hip
// the vote, the local key frames, the local points, the gather and the search (hs_localmap.hip); w: the carve of the call's d_work
const char* hs_local_map_search_why(const hs_kf_table* T, const int32_t* d_frame_lm, int n_assoc, const int32_t* d_neigh, int neigh_cap, const int32_t* d_parent,
                                    const hs_frame_view* F, const hs_landmark* d_lms, const hs_proj_params* pp, int cap, const hs_local_map_out* out,
                                    const HsLocalMapWork& w);
int hs_local_map_search_enqueue(hs_orb* h, const hs_kf_table* T, const int32_t* d_frame_lm, int n_assoc, const int32_t* d_neigh, int neigh_cap, const int32_t* d_parent,
                                int n_max_local_keyframes, int n_neighbor_keyframes, const hs_frame_view* F, const hs_pose_view* d_pose, const hs_landmark* d_lms,
                                const hs_proj_params* pp, int cap, const hs_local_map_out* out, const HsLocalMapWork& w, hipStream_t s);

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

// ---- the optimiser tail of a track stage (motion model, local map, reference key frame): the edges of the frame's associations, a gate
// where the stage has one, the optimiser, the discard of its outliers
struct HsPoseTail {
    int mode;                                                        // HS_TRACK_MOTION / HS_TRACK_LOCAL: what the discard does with an outlier
    hs_pose_problem* problem; hs_pose_edge* edges; uint8_t* outlier; hs_pose_result* pose;
    int32_t* n_edges;                                                // with a gate [2]: counted, then what the gate lets the optimiser see; without [1]
    const hs_track_result* gate_track; const hs_track_initial_result* gate_init;      // at most one of the two
    int32_t* count;                                                  // where the discard leaves its count
    int32_t* n_run() const { return n_edges + (gate_track || gate_init ? 1 : 0); }
};

// ---- the two track stages (hs_track.hip), which hs_track_frame_device and the calls of hs_track_initial.hip chain.  HsTrackPlan: the arguments every
// track stage takes and what the stages derive from them, formed once and read by the predicates and by the enqueues; the carve is integer arithmetic
struct HsTrackPlan {
    const hs_frame_view* F; const hs_kf_table* T; const hs_landmark* d_lms; const hs_track_params* tp; const hs_track_state* st; const hs_track_out* out;
    bool ok;                                                         // F, T, tp, st and d_work are there (otherwise: nothing derived, and refused)
    hs_frame_view Fs;                                                // F with the state's kp_lm_obs
    HsWorkCursor c; HsTrackWork w;
    hs_proj_params narrow, wide, local;
    static hs_proj_params proj(float th, float ratio, const hs_track_params& tp, bool last_frame)
    {
        hs_proj_params pp{};
        pp.th = th; pp.score_threshold = tp.th_high; pp.second_best_ratio = ratio; pp.frac_smaller = 0.5f; pp.frac_larger = 1.5f;
        pp.use_distance = last_frame ? 0 : 1; pp.use_stereo = 1; pp.check_rotation = last_frame ? 1 : 0; pp.use_prev_matched = 1;
        pp.max_view_angle = 1.047f; pp.reproj_threshold = 5.99f; pp.sigma_ref = tp.sigma_ref;
        return pp;
    }
    HsTrackPlan(const hs_frame_view* F, const hs_kf_table* T, const hs_landmark* d_lms, const hs_track_params* tp, const hs_track_state* st, const hs_track_out* out,
                void* d_work)
        : F(F), T(T), d_lms(d_lms), tp(tp), st(st), out(out), ok(F && T && tp && st && d_work), Fs(ok ? *F : hs_frame_view{}), c(ok ? d_work : nullptr),
          w(c, Fs.n, ok ? T->L : 0), narrow{}, wide{}, local{}
    {
        if (!ok) return;
        Fs.kp_lm_obs = st->kp_lm_obs;
        narrow = proj(tp->th_motion, tp->nnratio_motion, *tp, true); wide = proj(tp->th_motion_wide, tp->nnratio_motion, *tp, true);
        local = proj(tp->th_local, tp->nnratio_local, *tp, false);
    }
};
inline const char* hs_pose_tail_why(const HsPoseTail& t, const HsTrackPlan& p)
{
    const int n = p.Fs.n;
    return hs_first({ hs_pose_edges_why(&p.Fs, p.d_lms, p.T->L, p.st->kp_lm, t.edges, n, t.n_edges), hs_pose_optimize_why(1, t.problem, nullptr, t.n_run(), n, t.edges, t.pose),
                      hs_track_discard_why(t.mode, t.edges, t.n_run(), n, t.outlier, t.pose, p.T, p.st->kp_lm, p.st->kp_outl, p.st->n_matches, t.count) });
}
inline void hs_pose_tail_enqueue(const HsPoseTail& t, const HsTrackPlan& p, hipStream_t s)
{
    const int n = p.Fs.n; const hs_track_state* st = p.st;
    hs_launch_pose_edges(p.Fs, p.d_lms, p.T->L, st->kp_lm, p.tp->sigma_ref, t.edges, n, t.n_edges, s);
    if (t.gate_track) hs_launch_track_gate(t.gate_track, t.n_edges, s);
    if (t.gate_init) hs_launch_init_edges_gate(t.gate_init, t.n_edges, s);
    hs_launch_pose_optimize(1, t.problem, nullptr, t.n_run(), n, t.edges, t.outlier, t.pose, s);
    hs_launch_track_discard(t.mode, t.edges, t.n_run(), n, t.outlier, t.pose, *p.T, p.Fs.sensor, n, st->kp_lm, st->kp_outl, st->n_matches, t.count, s);
}
const char* hs_track_motion_why(const HsTrackPlan& p, const float* d_Tcw_pred, const hs_keypoint* d_last_kps, const int32_t* d_last_kp_lm, int n_last);
int hs_track_motion_enqueue(hs_orb* h, const HsTrackPlan& p, const float* d_Tcw_pred, const hs_keypoint* d_last_kps, const int32_t* d_last_kp_lm, int n_last, hipStream_t s);
const char* hs_track_local_why(const HsTrackPlan& p, const float* d_Tcw_in, const int32_t* d_neigh, int neigh_cap, const int32_t* d_parent, int cap);
int hs_track_local_enqueue(hs_orb* h, const HsTrackPlan& p, const float* d_Tcw_in, const int32_t* d_neigh, int neigh_cap, const int32_t* d_parent, int cap, hipStream_t s);
