// hs_track.hip — entry points of the resident tracking chain (include/hyslam_amd.h): hs_pose_views_device, hs_frame_associate_device,
// hs_frame_views_device, hs_track_discard_device, and the two strategies hs_track_motion_model_device / hs_track_local_map_device with
// hs_track_frame_device, which are the existing device calls and the glue kernels of kernels_track.hip enqueued on one stream.  Nothing here
// synchronises, reads device memory or claims the handle's scratch (the projection search's grid lists excepted, as in hs_local_map_search_device).
#include "hs_track.h"
#include <cstddef>

namespace {
hs_proj_params proj_params(float th, float ratio, const hs_track_params& tp, bool last_frame)
{
    hs_proj_params pp{};
    pp.th = th; pp.score_threshold = tp.th_high; pp.second_best_ratio = ratio; pp.frac_smaller = 0.5f; pp.frac_larger = 1.5f;
    pp.use_distance = last_frame ? 0 : 1; pp.use_stereo = 1; pp.check_rotation = last_frame ? 1 : 0; pp.use_prev_matched = 1;
    pp.max_view_angle = 1.047f; pp.reproj_threshold = 5.99f; pp.sigma_ref = tp.sigma_ref;
    return pp;
}
}  // namespace

extern "C" {

size_t hs_track_work_bytes(int n, int n_last, int L, int cap) { (void)n_last; (void)cap; return HsTrackWork::bytes(n, L); }

int hs_device_alloc(hs_orb* h, size_t bytes, void** out)
{
    if (!h) return HS_ERR_INVALID;
    if (!out) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    *out = nullptr;
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    HIP_TRY(h, hipMalloc(out, std::max<size_t>(bytes, 16)));
    HIP_TRY(h, hs_poison_fresh(*out, std::max<size_t>(bytes, 16)));
    return HS_OK;
}

int hs_device_free(hs_orb* h, void* d_ptr)
{
    if (!h) return HS_ERR_INVALID;
    if (!d_ptr) return HS_OK;
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    HIP_TRY(h, hipFree(d_ptr));
    return HS_OK;
}

int hs_device_copy(hs_orb* h, void* dst, const void* src, size_t bytes, int kind, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if ((kind != 1 && kind != 2) || (bytes > 0 && (!dst || !src))) return hs_fail(h, HS_ERR_INVALID, "bad argument (kind: 1 host to device, 2 device to host)");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    HIP_TRY(h, hipStreamSynchronize(hs_stream_or(h, stream)));
    if (bytes > 0) HIP_TRY(h, hipMemcpy(dst, src, bytes, kind == 1 ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
    return HS_OK;
}

int hs_pose_views_device(hs_orb* h, const float* d_Tcw, hs_pose_view* d_out, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!d_Tcw || !d_out) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    hs_launch_pose_view(d_Tcw, d_out, nullptr, nullptr, hs_stream_or(h, stream));
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_frame_associate_device(hs_orb* h, int n, int L, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, int n_ops, const int32_t* d_op_view,
                              const int32_t* d_op_lm, void* d_work, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (n < 0 || L < 0 || n_ops < 0 || !d_n_matches || !d_work || (n > 0 && (!d_kp_lm || !d_kp_outl)) || (n_ops > 0 && (!d_op_view || !d_op_lm)))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    HsWorkCursor c(d_work);
    hs_launch_frame_associate(n, L, d_kp_lm, d_kp_outl, d_n_matches, n_ops, d_op_view, d_op_lm, HsAssocWork(c, n, L), hs_stream_or(h, stream));
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_frame_views_device(hs_orb* h, int n, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, const hs_kf_table* T, int drop_bad, int32_t* d_kp_lm_obs,
                          void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (n < 0 || n > 65535 || !T || T->L < 0 || (n > 0 && (!d_kp_lm || !d_kp_lm_obs)) || (T->L > 0 && !T->lm_nobs) ||
        (drop_bad && (!d_kp_outl || !d_n_matches || (T->L > 0 && !T->lm_bad))))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    hs_launch_frame_views(n, d_kp_lm, d_kp_outl, d_n_matches, *T, drop_bad ? 1 : 0, d_kp_lm_obs, hs_stream_or(h, stream));
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

// n: the frame's keypoint count bounds edges[k].kp; the public form has no frame, so an edge may name any view below 65536 (hs_frame_view's limit)
int hs_track_discard_device(hs_orb* h, int mode, const hs_pose_edge* d_edges, const int32_t* d_n_edges, int edge_cap, const uint8_t* d_outlier,
                            const hs_pose_result* d_result, const hs_kf_table* T, int sensor, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches,
                            int32_t* d_counts, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if ((mode != HS_TRACK_MOTION && mode != HS_TRACK_LOCAL) || !d_n_edges || edge_cap < 0 || !d_result || !T || T->L < 0 || (T->L > 0 && !T->lm_nobs) || !d_n_matches ||
        !d_counts || (edge_cap > 0 && (!d_edges || !d_outlier || !d_kp_lm || !d_kp_outl)))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    hs_launch_track_discard(mode, d_edges, d_n_edges, edge_cap, d_outlier, d_result, *T, sensor, 65536, d_kp_lm, d_kp_outl, d_n_matches, d_counts,
                            hs_stream_or(h, stream));
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_track_motion_model_device(hs_orb* h, const hs_frame_view* F, const float* d_Tcw_pred, const hs_keypoint* d_last_kps, const int32_t* d_last_kp_lm, int n_last,
                                 const hs_kf_table* T, const hs_landmark* d_lms, const hs_track_params* tp, const hs_track_state* st, const hs_track_out* out,
                                 void* d_work, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!F || F->n < 1 || F->n > 65535 || !F->kps || !F->desc || !d_Tcw_pred || n_last < 1 || !d_last_kps || !d_last_kp_lm || !T || T->L < 1 || !T->lm_nobs || !d_lms ||
        ((uintptr_t)d_lms & 15) || !tp || !state_ok(st) || !track_out_ok(out) || !d_work)
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    hipStream_t s = hs_stream_or(h, stream);
    const int n = F->n, L = T->L;
    HsWorkCursor c(d_work);
    const HsTrackWork w(c, n, L);
    hs_frame_view Fs = *F;
    Fs.kp_lm_obs = st->kp_lm_obs;
    hs_launch_pose_view(d_Tcw_pred, &out->pose_view[0], &out->problem[0], F, s);                                  // current_frame.SetPose(Tcw_cur)
    hs_launch_last_gather(d_lms, L, d_last_kp_lm, d_last_kps, n_last, out->last_lms, s);                          // LastFrame.replicatemvpMapPoints()
    hs_launch_track_clear(n, st->kp_lm, st->kp_outl, st->n_matches, st->kp_lm_obs, s);                            // clearAssociations()
    const hs_proj_params narrow = proj_params(tp->th_motion, tp->nnratio_motion, *tp, true), wide = proj_params(tp->th_motion_wide, tp->nnratio_motion, *tp, true);
    int rc = hs_search_by_projection_posed_device(h, &Fs, &out->pose_view[0], out->last_lms, n_last, &narrow, out->narrow_idx, out->narrow_dist, out->narrow_n, s);
    if (rc != HS_OK) return rc;
    rc = hs_search_by_projection_posed_device(h, &Fs, &out->pose_view[0], out->last_lms, n_last, &wide, out->wide_idx, out->wide_dist, out->wide_n, s);
    if (rc != HS_OK) return rc;
    hs_launch_track_select(n_last, out->narrow_idx, out->narrow_n, out->wide_idx, out->wide_n, tp->n_min_matches, out->op_view, out->result, s);
    hs_launch_frame_associate(n, L, st->kp_lm, st->kp_outl, st->n_matches, n_last, out->op_view, d_last_kp_lm, w.assoc, s);
    rc = hs_pose_edges_device(h, &Fs, d_lms, L, st->kp_lm, tp->sigma_ref, out->edges_motion, n, &out->n_edges_motion[0], nullptr, s);
    if (rc != HS_OK) return rc;
    hs_launch_track_gate(out->result, out->n_edges_motion, s);                                                     // `return -1` ahead of PoseOptimization
    rc = hs_pose_optimize_device(h, 1, &out->problem[0], nullptr, &out->n_edges_motion[1], n, out->edges_motion, out->outlier_motion, out->pose_motion, nullptr, s);
    if (rc != HS_OK) return rc;
    hs_launch_track_discard(HS_TRACK_MOTION, out->edges_motion, &out->n_edges_motion[1], n, out->outlier_motion, out->pose_motion, *T, F->sensor, n, st->kp_lm,
                            st->kp_outl, st->n_matches, &out->result->n_matches_map, s);
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_track_local_map_device(hs_orb* h, const hs_frame_view* F, const float* d_Tcw_in, const hs_kf_table* T, const hs_landmark* d_lms, const int32_t* d_neigh,
                              int neigh_cap, const int32_t* d_parent, int cap, const hs_track_params* tp, const hs_track_state* st, const hs_track_out* out,
                              void* d_work, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!F || F->n < 1 || F->n > 65535 || !F->kps || !F->desc || !d_Tcw_in || !T || T->L < 1 || !T->lm_nobs || !T->lm_bad || !d_lms || ((uintptr_t)d_lms & 15) || cap < 1 ||
        !tp || !state_ok(st) || !track_out_ok(out) || !d_work)
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    hipStream_t s = hs_stream_or(h, stream);
    const int n = F->n, L = T->L;
    HsWorkCursor c(d_work);
    const HsTrackWork w(c, n, L);
    hs_frame_view Fs = *F;
    Fs.kp_lm_obs = st->kp_lm_obs;
    hs_launch_pose_view(d_Tcw_in, &out->pose_view[1], &out->problem[1], F, s);
    hs_launch_frame_views(n, st->kp_lm, st->kp_outl, st->n_matches, *T, 1, st->kp_lm_obs, s);                     // SearchLocalPoints :56-67
    const hs_proj_params pp = proj_params(tp->th_local, tp->nnratio_local, *tp, false);
    int rc = hs_local_map_search_posed_device(h, T, st->kp_lm, n, d_neigh, neigh_cap, d_parent, tp->n_max_local_keyframes, tp->n_neighbor_keyframes, &Fs,
                                              &out->pose_view[1], d_lms, &pp, cap, &out->local, w.local_map.base, s);
    if (rc != HS_OK) return rc;
    hs_launch_frame_associate(n, L, st->kp_lm, st->kp_outl, st->n_matches, cap, out->local.match_idx, out->local.sel, w.assoc, s);
    rc = hs_pose_edges_device(h, &Fs, d_lms, L, st->kp_lm, tp->sigma_ref, out->edges_local, n, out->n_edges_local, nullptr, s);
    if (rc != HS_OK) return rc;
    rc = hs_pose_optimize_device(h, 1, &out->problem[1], nullptr, out->n_edges_local, n, out->edges_local, out->outlier_local, out->pose_local, nullptr, s);
    if (rc != HS_OK) return rc;
    hs_launch_track_discard(HS_TRACK_LOCAL, out->edges_local, out->n_edges_local, n, out->outlier_local, out->pose_local, *T, F->sensor, n, st->kp_lm, st->kp_outl,
                            st->n_matches, &out->result->n_inliers, s);
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_track_frame_device(hs_orb* h, const hs_frame_view* F, const float* d_Tcw_pred, const hs_keypoint* d_last_kps, const int32_t* d_last_kp_lm, int n_last,
                          const hs_kf_table* T, const hs_landmark* d_lms, const int32_t* d_neigh, int neigh_cap, const int32_t* d_parent, int cap,
                          const hs_track_params* tp, const hs_track_state* st, const hs_track_out* out, void* d_work, void* stream)
{
    const int rc = hs_track_motion_model_device(h, F, d_Tcw_pred, d_last_kps, d_last_kp_lm, n_last, T, d_lms, tp, st, out, d_work, stream);
    if (rc != HS_OK) return rc;
    return hs_track_local_map_device(h, F, out->pose_motion->Tcw, T, d_lms, d_neigh, neigh_cap, d_parent, cap, tp, st, out, d_work, stream);
}

}  // extern "C"
