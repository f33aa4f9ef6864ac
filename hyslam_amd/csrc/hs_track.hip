// hs_track.hip — entry points of the resident tracking chain (include/hyslam_amd.h): hs_pose_views_device, hs_frame_associate_device,
// hs_frame_views_device, hs_track_discard_device, and the two strategies hs_track_motion_model_device / hs_track_local_map_device with
// hs_track_frame_device, which are the existing stages and the glue kernels of kernels_track.hip enqueued on one stream: a chain's predicate is its
// stages' predicates (hs_track.h) on what its enqueue hands them.  Nothing here synchronises, reads device memory or claims the handle's scratch (the
// projection search's grid lists excepted, as in hs_local_map_search_device).
#include "hs_track.h"
#include <cstddef>

namespace {
HsPoseTail motion_tail(const hs_track_out* o)      // the gate: `return -1` ahead of PoseOptimization
{
    return HsPoseTail{ HS_TRACK_MOTION, &o->problem[0], o->edges_motion, o->outlier_motion, o->pose_motion, o->n_edges_motion, o->result, nullptr, &o->result->n_matches_map };
}
HsPoseTail local_tail(const hs_track_out* o)
{
    return HsPoseTail{ HS_TRACK_LOCAL, &o->problem[1], o->edges_local, o->outlier_local, o->pose_local, o->n_edges_local, nullptr, nullptr, &o->result->n_inliers };
}
// beside the plan's structs: what the glue kernels read that are no entry point of their own (k_last_gather, k_track_clear, k_track_select, k_track_gate)
bool track_shape_ok(const HsTrackPlan& p)
{
    return p.ok && p.T->L >= 1 && p.d_lms && !((uintptr_t)p.d_lms & 15) && state_ok(p.st) && track_out_ok(p.out);
}
}  // namespace

const char* hs_track_motion_why(const HsTrackPlan& p, const float* d_Tcw_pred, const hs_keypoint* d_last_kps, const int32_t* d_last_kp_lm, int n_last)
{
    if (!track_shape_ok(p) || !d_last_kps || !d_last_kp_lm) return "bad argument";
    const hs_track_state* st = p.st; const hs_track_out* out = p.out;
    return hs_first({ hs_pose_views_why(d_Tcw_pred, &out->pose_view[0]),
                      hs_search_by_projection_why(&p.Fs, out->last_lms, n_last, &p.narrow, out->narrow_idx, out->narrow_dist, out->narrow_n),
                      hs_search_by_projection_why(&p.Fs, out->last_lms, n_last, &p.wide, out->wide_idx, out->wide_dist, out->wide_n),
                      hs_frame_associate_why(p.Fs.n, p.T->L, st->kp_lm, st->kp_outl, st->n_matches, n_last, out->op_view, d_last_kp_lm, p.w.assoc.base),
                      hs_pose_tail_why(motion_tail(out), p) });
}
int hs_track_motion_enqueue(hs_orb* h, const HsTrackPlan& p, const float* d_Tcw_pred, const hs_keypoint* d_last_kps, const int32_t* d_last_kp_lm, int n_last, hipStream_t s)
{
    const hs_track_state* st = p.st; const hs_track_out* out = p.out;
    const int n = p.Fs.n, L = p.T->L;
    hs_launch_pose_view(d_Tcw_pred, &out->pose_view[0], &out->problem[0], p.F, s);                                // current_frame.SetPose(Tcw_cur)
    hs_launch_last_gather(p.d_lms, L, d_last_kp_lm, d_last_kps, n_last, out->last_lms, s);                        // LastFrame.replicatemvpMapPoints()
    hs_launch_track_clear(n, st->kp_lm, st->kp_outl, st->n_matches, st->kp_lm_obs, s);                            // clearAssociations()
    int rc = hs_search_by_projection_enqueue(h, &p.Fs, &out->pose_view[0], out->last_lms, n_last, &p.narrow, out->narrow_idx, out->narrow_dist, out->narrow_n, s);
    if (rc == HS_OK) rc = hs_search_by_projection_enqueue(h, &p.Fs, &out->pose_view[0], out->last_lms, n_last, &p.wide, out->wide_idx, out->wide_dist, out->wide_n, s);
    if (rc != HS_OK) return rc;
    hs_launch_track_select(n_last, out->narrow_idx, out->narrow_n, out->wide_idx, out->wide_n, p.tp->n_min_matches, out->op_view, out->result, s);
    hs_launch_frame_associate(n, L, st->kp_lm, st->kp_outl, st->n_matches, n_last, out->op_view, d_last_kp_lm, p.w.assoc, s);
    hs_pose_tail_enqueue(motion_tail(out), p, s);
    return HS_OK;
}

const char* hs_track_local_why(const HsTrackPlan& p, const float* d_Tcw_in, const int32_t* d_neigh, int neigh_cap, const int32_t* d_parent, int cap)
{
    if (!track_shape_ok(p)) return "bad argument";
    const hs_track_state* st = p.st; const hs_track_out* out = p.out;
    const int n = p.Fs.n;
    return hs_first({ hs_pose_views_why(d_Tcw_in, &out->pose_view[1]), hs_frame_views_why(n, st->kp_lm, st->kp_outl, st->n_matches, p.T, 1, st->kp_lm_obs),
                      hs_local_map_search_why(p.T, st->kp_lm, n, d_neigh, neigh_cap, d_parent, &p.Fs, p.d_lms, &p.local, cap, &out->local, p.w.local_map),
                      hs_frame_associate_why(n, p.T->L, st->kp_lm, st->kp_outl, st->n_matches, cap, out->local.match_idx, out->local.sel, p.w.assoc.base),
                      hs_pose_tail_why(local_tail(out), p) });
}
int hs_track_local_enqueue(hs_orb* h, const HsTrackPlan& p, const float* d_Tcw_in, const int32_t* d_neigh, int neigh_cap, const int32_t* d_parent, int cap, hipStream_t s)
{
    const hs_track_state* st = p.st; const hs_track_out* out = p.out;
    const int n = p.Fs.n;
    hs_launch_pose_view(d_Tcw_in, &out->pose_view[1], &out->problem[1], p.F, s);
    hs_launch_frame_views(n, st->kp_lm, st->kp_outl, st->n_matches, *p.T, 1, st->kp_lm_obs, s);                   // SearchLocalPoints :56-67
    const int rc = hs_local_map_search_enqueue(h, p.T, st->kp_lm, n, d_neigh, neigh_cap, d_parent, p.tp->n_max_local_keyframes, p.tp->n_neighbor_keyframes, &p.Fs,
                                               &out->pose_view[1], p.d_lms, &p.local, cap, &out->local, p.w.local_map, s);
    if (rc != HS_OK) return rc;
    hs_launch_frame_associate(n, p.T->L, st->kp_lm, st->kp_outl, st->n_matches, cap, out->local.match_idx, out->local.sel, p.w.assoc, s);
    hs_pose_tail_enqueue(local_tail(out), p, s);
    return HS_OK;
}

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
    return hs_device_call(h, hs_pose_views_why(d_Tcw, d_out), stream, [&](hipStream_t s) { hs_launch_pose_view(d_Tcw, d_out, nullptr, nullptr, s); });
}

int hs_frame_associate_device(hs_orb* h, int n, int L, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, int n_ops, const int32_t* d_op_view,
                              const int32_t* d_op_lm, void* d_work, void* stream)
{
    return hs_device_call(h, hs_frame_associate_why(n, L, d_kp_lm, d_kp_outl, d_n_matches, n_ops, d_op_view, d_op_lm, d_work), stream, [&](hipStream_t s) {
        HsWorkCursor c(d_work);
        hs_launch_frame_associate(n, L, d_kp_lm, d_kp_outl, d_n_matches, n_ops, d_op_view, d_op_lm, HsAssocWork(c, n, L), s);
    });
}

int hs_frame_views_device(hs_orb* h, int n, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, const hs_kf_table* T, int drop_bad, int32_t* d_kp_lm_obs,
                          void* stream)
{
    return hs_device_call(h, hs_frame_views_why(n, d_kp_lm, d_kp_outl, d_n_matches, T, drop_bad, d_kp_lm_obs), stream,
                          [&](hipStream_t s) { hs_launch_frame_views(n, d_kp_lm, d_kp_outl, d_n_matches, *T, drop_bad ? 1 : 0, d_kp_lm_obs, s); });
}

// n: the frame's keypoint count bounds edges[k].kp; the public form has no frame, so an edge may name any view below 65536 (hs_frame_view's limit)
int hs_track_discard_device(hs_orb* h, int mode, const hs_pose_edge* d_edges, const int32_t* d_n_edges, int edge_cap, const uint8_t* d_outlier,
                            const hs_pose_result* d_result, const hs_kf_table* T, int sensor, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches,
                            int32_t* d_counts, void* stream)
{
    return hs_device_call(h, hs_track_discard_why(mode, d_edges, d_n_edges, edge_cap, d_outlier, d_result, T, d_kp_lm, d_kp_outl, d_n_matches, d_counts), stream,
                          [&](hipStream_t s) {
        hs_launch_track_discard(mode, d_edges, d_n_edges, edge_cap, d_outlier, d_result, *T, sensor, 65536, d_kp_lm, d_kp_outl, d_n_matches, d_counts, s);
    });
}

int hs_track_motion_model_device(hs_orb* h, const hs_frame_view* F, const float* d_Tcw_pred, const hs_keypoint* d_last_kps, const int32_t* d_last_kp_lm, int n_last,
                                 const hs_kf_table* T, const hs_landmark* d_lms, const hs_track_params* tp, const hs_track_state* st, const hs_track_out* out,
                                 void* d_work, void* stream)
{
    const HsTrackPlan p(F, T, d_lms, tp, st, out, d_work);
    return hs_device_call(h, hs_track_motion_why(p, d_Tcw_pred, d_last_kps, d_last_kp_lm, n_last), stream,
                          [&](hipStream_t s) { return hs_track_motion_enqueue(h, p, d_Tcw_pred, d_last_kps, d_last_kp_lm, n_last, s); });
}

int hs_track_local_map_device(hs_orb* h, const hs_frame_view* F, const float* d_Tcw_in, const hs_kf_table* T, const hs_landmark* d_lms, const int32_t* d_neigh,
                              int neigh_cap, const int32_t* d_parent, int cap, const hs_track_params* tp, const hs_track_state* st, const hs_track_out* out,
                              void* d_work, void* stream)
{
    const HsTrackPlan p(F, T, d_lms, tp, st, out, d_work);
    return hs_device_call(h, hs_track_local_why(p, d_Tcw_in, d_neigh, neigh_cap, d_parent, cap), stream,
                          [&](hipStream_t s) { return hs_track_local_enqueue(h, p, d_Tcw_in, d_neigh, neigh_cap, d_parent, cap, s); });
}

int hs_track_frame_device(hs_orb* h, const hs_frame_view* F, const float* d_Tcw_pred, const hs_keypoint* d_last_kps, const int32_t* d_last_kp_lm, int n_last,
                          const hs_kf_table* T, const hs_landmark* d_lms, const int32_t* d_neigh, int neigh_cap, const int32_t* d_parent, int cap,
                          const hs_track_params* tp, const hs_track_state* st, const hs_track_out* out, void* d_work, void* stream)
{
    const HsTrackPlan p(F, T, d_lms, tp, st, out, d_work);
    const char* why = hs_track_motion_why(p, d_Tcw_pred, d_last_kps, d_last_kp_lm, n_last);
    if (!why) why = hs_track_local_why(p, out->pose_motion->Tcw, d_neigh, neigh_cap, d_parent, cap);
    return hs_device_call(h, why, stream, [&](hipStream_t s) {
        const int rc = hs_track_motion_enqueue(h, p, d_Tcw_pred, d_last_kps, d_last_kp_lm, n_last, s);
        return rc != HS_OK ? rc : hs_track_local_enqueue(h, p, out->pose_motion->Tcw, d_neigh, neigh_cap, d_parent, cap, s);
    });
}

}  // extern "C"
