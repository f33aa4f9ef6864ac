// hs_track_initial.hip — TrackingStateNormal::initialPoseEstimation as one enqueue-only call (include/hyslam_amd.h, "initial pose estimation as one
// resident call"): hs_track_reference_keyframe_device, hs_track_initial_device and hs_track_normal_device.  Each is the existing device calls and the
// gate kernels of kernels_track_initial.hip enqueued on one stream; the arguments of the whole sequence are checked before its first launch; nothing
// here synchronises, reads device memory or claims the handle's scratch (the motion and local stages' projection searches take their grid lists).
#include "hs_track.h"
#include <cstddef>

namespace {
bool iout_ok(const hs_track_initial_out* o, bool frame_result)
{
    return o && o->bow_word && o->bow_weight && o->bow_node && o->match_kf && o->op_view && o->op_lm && o->pose_view && o->problem && o->edges && o->outlier &&
           o->n_edges && o->pose && o->Tcw_init && o->result && (!frame_result || o->frame_result) && !((uintptr_t)o->edges & 15);
}
// everything hs_track_reference_keyframe_device and the calls it is made of refuse
bool refkf_ok(const hs_frame_view* F, const hs_vocab_dev* vocab, const hs_kf_features* K, const int32_t* d_kf_slot, int kf_cap, const float* d_Tcw_last,
              const hs_kf_table* T, const hs_landmark* d_lms, const hs_track_params* tp, const hs_track_refkf_params* rp, const hs_track_state* st,
              const hs_track_initial_out* iout, bool frame_result, const void* d_work)
{
    return F && F->n >= 1 && F->n <= 65535 && F->kps && F->desc && vocab && feats_ok(K) && d_kf_slot && kf_cap >= 1 && d_Tcw_last && T && T->L >= 1 && T->lm_nobs &&
           T->lm_bad && d_lms && !((uintptr_t)d_lms & 15) && tp && rp && state_ok(st) && iout_ok(iout, frame_result) && d_work;
}
// what the motion stage refuses beyond that (hs_track_motion_model_device checks its `out` itself, before its first launch)
bool motion_ok(const float* d_Tcw_pred, const hs_keypoint* d_last_kps, const int32_t* d_last_kp_lm, int n_last, const hs_track_out* out)
{
    return d_Tcw_pred && d_last_kps && d_last_kp_lm && n_last >= 1 && track_out_ok(out);
}

int refkf_enqueue(hs_orb* h, const hs_frame_view* F, const hs_vocab_dev* vocab, const hs_kf_features* K, const int32_t* d_kf_slot, int kf_cap, const float* d_Tcw_last,
                  const float* d_Tcw_entry, const hs_track_result* d_motion, const hs_kf_table* T, const hs_landmark* d_lms, const hs_track_params* tp,
                  const hs_track_refkf_params* rp, const hs_track_state* st, const hs_track_initial_out* o, void* d_work, hipStream_t s)
{
    const int n = F->n, L = T->L;
    HsWorkCursor c(d_work);
    const HsInitialWork w(c, n, L);
    hs_frame_view Fs = *F;
    Fs.kp_lm_obs = st->kp_lm_obs;
    int rc = hs_bow_transform_device(h, vocab, F->desc, nullptr, n, o->bow_word, o->bow_weight, o->bow_node, s);                          // Frame::ComputeBoW
    if (rc != HS_OK) return rc;
    rc = hs_search_by_bow_kf_device(h, K, d_kf_slot, T, F->kps, F->desc, o->bow_node, o->bow_weight, n, rp->th_low, rp->nnratio, o->match_kf, kf_cap, o->op_view, o->op_lm,
                                    &o->result->n_bow, nullptr, s);
    if (rc != HS_OK) return rc;
    hs_launch_init_gate(n, d_motion, *rp, o->op_view, o->op_lm, w.op_view_run, w.op_lm_run, o->result, s);            // both `if`s, as one status
    hs_launch_frame_associate_views(n, L, st->kp_lm, st->kp_outl, st->n_matches, w.op_view_run, w.op_lm_run, w.vassoc, s);                // associateLandMarks
    hs_launch_pose_view(d_Tcw_last, o->pose_view, o->problem, F, s);                                                                      // SetPose(last_frame.mTcw)
    rc = hs_pose_edges_device(h, &Fs, d_lms, L, st->kp_lm, tp->sigma_ref, o->edges, n, &o->n_edges[0], nullptr, s);
    if (rc != HS_OK) return rc;
    hs_launch_init_edges_gate(o->result, o->n_edges, s);
    rc = hs_pose_optimize_device(h, 1, o->problem, nullptr, &o->n_edges[1], n, o->edges, o->outlier, o->pose, nullptr, s);
    if (rc != HS_OK) return rc;
    hs_launch_track_discard(HS_TRACK_MOTION, o->edges, &o->n_edges[1], n, o->outlier, o->pose, *T, F->sensor, n, st->kp_lm, st->kp_outl, st->n_matches,
                            &o->result->n_matches_map_refkf, s);
    hs_launch_init_finish(d_motion, rp->thresh_init, o->pose, d_Tcw_entry, o->Tcw_init, o->result, s);
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}
}  // namespace

extern "C" {

size_t hs_track_initial_work_bytes(int n, int n_last, int L, int cap, int kf_cap) { (void)n_last; (void)cap; (void)kf_cap; return HsInitialWork::bytes(n, L); }

int hs_track_reference_keyframe_device(hs_orb* h, const hs_frame_view* F, const hs_vocab_dev* vocab, const hs_kf_features* K, const int32_t* d_kf_slot, int kf_cap,
                                       const float* d_Tcw_last, const float* d_Tcw_entry, const hs_track_result* d_motion_result, const hs_kf_table* T,
                                       const hs_landmark* d_lms, const hs_track_params* tp, const hs_track_refkf_params* rp, const hs_track_state* st,
                                       const hs_track_initial_out* iout, void* d_work, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!refkf_ok(F, vocab, K, d_kf_slot, kf_cap, d_Tcw_last, T, d_lms, tp, rp, st, iout, false, d_work) || !d_Tcw_entry) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    return refkf_enqueue(h, F, vocab, K, d_kf_slot, kf_cap, d_Tcw_last, d_Tcw_entry, d_motion_result, T, d_lms, tp, rp, st, iout, d_work, hs_stream_or(h, stream));
}

int hs_track_initial_device(hs_orb* h, const hs_frame_view* F, int velocity_valid, const float* d_Tcw_pred, const hs_keypoint* d_last_kps, const int32_t* d_last_kp_lm,
                            int n_last, const hs_vocab_dev* vocab, const hs_kf_features* K, const int32_t* d_kf_slot, int kf_cap, const float* d_Tcw_last,
                            const float* d_Tcw_entry, const hs_kf_table* T, const hs_landmark* d_lms, const hs_track_params* tp, const hs_track_refkf_params* rp,
                            const hs_track_state* st, const hs_track_out* out, const hs_track_initial_out* iout, void* d_work, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!refkf_ok(F, vocab, K, d_kf_slot, kf_cap, d_Tcw_last, T, d_lms, tp, rp, st, iout, false, d_work) ||
        (velocity_valid ? !motion_ok(d_Tcw_pred, d_last_kps, d_last_kp_lm, n_last, out) : !d_Tcw_entry))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    hipStream_t s = hs_stream_or(h, stream);
    if (!velocity_valid) return refkf_enqueue(h, F, vocab, K, d_kf_slot, kf_cap, d_Tcw_last, d_Tcw_entry, nullptr, T, d_lms, tp, rp, st, iout, d_work, s);
    const int rc = hs_track_motion_model_device(h, F, d_Tcw_pred, d_last_kps, d_last_kp_lm, n_last, T, d_lms, tp, st, out, d_work, s);   // HsTrackWork heads the area
    if (rc != HS_OK) return rc;
    return refkf_enqueue(h, F, vocab, K, d_kf_slot, kf_cap, d_Tcw_last, out->pose_motion->Tcw, out->result, T, d_lms, tp, rp, st, iout, d_work, s);
}

int hs_track_normal_device(hs_orb* h, const hs_frame_view* F, int velocity_valid, const float* d_Tcw_pred, const hs_keypoint* d_last_kps, const int32_t* d_last_kp_lm,
                           int n_last, const hs_vocab_dev* vocab, const hs_kf_features* K, const int32_t* d_kf_slot, int kf_cap, const float* d_Tcw_last,
                           const float* d_Tcw_entry, const hs_kf_table* T, const hs_landmark* d_lms, const int32_t* d_neigh, int neigh_cap, const int32_t* d_parent, int cap,
                           const hs_track_params* tp, const hs_track_refkf_params* rp, const hs_track_state* st, const hs_track_out* out,
                           const hs_track_initial_out* iout, void* d_work, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    // the local stage's own refusals (cap, its `out`) would come after the initial stage was enqueued: made here
    if (!refkf_ok(F, vocab, K, d_kf_slot, kf_cap, d_Tcw_last, T, d_lms, tp, rp, st, iout, true, d_work) || cap < 1 || !track_out_ok(out) ||
        iout->frame_result == out->result)
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    int rc = hs_track_initial_device(h, F, velocity_valid, d_Tcw_pred, d_last_kps, d_last_kp_lm, n_last, vocab, K, d_kf_slot, kf_cap, d_Tcw_last, d_Tcw_entry, T, d_lms, tp,
                                     rp, st, out, iout, d_work, stream);
    if (rc != HS_OK) return rc;
    rc = hs_track_local_map_device(h, F, iout->Tcw_init, T, d_lms, d_neigh, neigh_cap, d_parent, cap, tp, st, out, d_work, stream);
    if (rc != HS_OK) return rc;
    hs_launch_frame_result(velocity_valid ? out->result : nullptr, iout->result, &out->result->n_inliers, iout->frame_result, hs_stream_or(h, stream));
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

}  // extern "C"
