// hs_keyframe.hip — entry points of the stages that follow the two track functions (include/hyslam_amd.h, "after the two track functions"):
// hs_keyframe_reference_device, _gate_, _clean_, _need_, _create_, _discard_ and hs_track_keyframe_device, which is these six in this order.  Each is
// the existing device calls and the kernels of kernels_keyframe.hip enqueued on one stream; nothing here synchronises or reads device memory.
#include "hs_track.h"
#include <cstddef>

namespace {
bool n_ok(int n) { return n >= 1 && n <= 65535; }
bool table_ok(const hs_kf_table* T) { return T && T->L >= 0 && (T->L == 0 || (T->lm_nobs && T->lm_bad)); }
// what stage 1's vote reads beyond that: hs_kf_votes_device would refuse it only after the launches before it
bool vote_table_ok(const hs_kf_table* T) { return table_ok(T) && T->n_kf >= 0 && T->lm_obs_offsets && (T->n_kf == 0 || (T->kf_bad && T->kf_id)); }
bool out_ok(const hs_keyframe_out* o, int new_cap)
{
    return o && new_cap >= 0 && o->result && o->pose_view && o->obs_offsets && o->desc_offsets && (!o->lms || (o->lms_cap >= 0 && !((uintptr_t)o->lms & 15))) &&
           (new_cap == 0 || (o->new_view && o->new_pos && o->entries && o->obs && o->desc && o->lm_index));
}
}  // namespace

extern "C" {

size_t hs_keyframe_work_bytes(int n, int kf_cap, int new_cap) { (void)new_cap; return HsKeyframeWork::bytes(n, kf_cap); }

int hs_keyframe_reference_device(hs_orb* h, int n, const hs_track_state* st, const hs_kf_table* T, int32_t* d_ref_slot, hs_keyframe_result* d_result, void* d_work,
                                 void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!n_ok(n) || !state_ok(st) || !vote_table_ok(T) || !d_ref_slot || !d_result || !d_work) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    hipStream_t s = hs_stream_or(h, stream);
    HsWorkCursor c(d_work);
    const HsKeyframeWork w(c, n, T->n_kf);                       // the caller's kf_cap is at least T->n_kf (HsKeyframeWork)
    hs_launch_kfd_ref_begin(n, w.q_off, s);
    int rc = hs_frame_views_device(h, n, st->kp_lm, st->kp_outl, st->n_matches, T, 1, st->kp_lm_obs, s);                // removeLandMarkAssociation of bad landmarks (:290)
    if (rc != HS_OK) return rc;
    rc = hs_kf_votes_device(h, T, 1, w.q_off, st->kp_lm, nullptr, 1, 0, w.weights, &w.vote[0], &w.vote[1], nullptr, nullptr, 0, &w.vote[2], s);
    if (rc != HS_OK) return rc;
    hs_launch_kfd_ref_update(&w.vote[0], d_ref_slot, d_result, s);
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_keyframe_gate_device(hs_orb* h, const hs_track_result* d_track_result, const hs_keyframe_params* prm, hs_keyframe_result* d_result, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!prm || !d_result || (prm->ok_override < 0 && !d_track_result)) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    hs_launch_kfd_gate(d_track_result, *prm, d_result, hs_stream_or(h, stream));
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_keyframe_clean_device(hs_orb* h, int n, const hs_track_state* st, const hs_kf_table* T, hs_keyframe_result* d_result, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!n_ok(n) || !state_ok(st) || !table_ok(T) || !d_result) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    hs_launch_kfd_clean(n, *st, *T, d_result, hs_stream_or(h, stream));
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_keyframe_need_device(hs_orb* h, int n, int sensor, const float* d_depth, const hs_track_state* st, const hs_kf_table* T, const hs_kf_features* K,
                            const int32_t* d_ref_slot, const hs_track_result* d_track_result, const hs_keyframe_params* prm, hs_keyframe_result* d_result, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!n_ok(n) || (sensor != 0 && !d_depth) || !state_ok(st) || !table_ok(T) || !K || K->n_kf < 0 || (K->n_kf > 0 && (!K->kf_off || !K->kp_lm)) || !d_ref_slot || !prm ||
        !d_result)
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    hs_launch_kfd_need(n, sensor, d_depth, *st, *T, *K, d_ref_slot, d_track_result, *prm, d_result, hs_stream_or(h, stream));
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_keyframe_create_device(hs_orb* h, const hs_frame_view* F, const float* d_depth, const float* d_Tcw, const hs_track_state* st, const hs_kf_table* T,
                              const hs_keyframe_params* prm, int new_cap, const hs_keyframe_out* out, void* d_work, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!F || !n_ok(F->n) || !F->kps || !F->desc || !d_depth || !d_Tcw || !state_ok(st) || !table_ok(T) || !prm || !out_ok(out, new_cap) || !d_work)
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    hipStream_t s = hs_stream_or(h, stream);
    const int rc = hs_pose_views_device(h, d_Tcw, out->pose_view, s);                                                  // current_frame.UpdatePoseMatrices() (:32)
    if (rc != HS_OK) return rc;
    HsWorkCursor c(d_work);
    hs_launch_kfd_create(*F, d_depth, *st, *T, *prm, new_cap, *out, HsKeyframeWork(c, F->n, T->n_kf).keys, s);
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_keyframe_discard_device(hs_orb* h, int n, const hs_track_state* st, hs_keyframe_result* d_result, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!n_ok(n) || !state_ok(st) || !d_result) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    hs_launch_kfd_discard(n, *st, d_result, hs_stream_or(h, stream));
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_track_keyframe_device(hs_orb* h, const hs_frame_view* F, const float* d_depth, const float* d_Tcw, const hs_kf_table* T, const hs_kf_features* K,
                             const hs_track_result* d_track_result, const hs_keyframe_params* prm, const hs_track_state* st, int32_t* d_ref_slot, int new_cap,
                             const hs_keyframe_out* out, void* d_work, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    // every stage's arguments before the first launch
    if (!F || !n_ok(F->n) || !F->kps || !F->desc || !d_depth || !d_Tcw || !state_ok(st) || !vote_table_ok(T) || !K || K->n_kf < 0 || (K->n_kf > 0 && (!K->kf_off || !K->kp_lm)) ||
        !prm || (prm->ok_override < 0 && !d_track_result) || !d_ref_slot || !out_ok(out, new_cap) || !d_work)
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    int rc = hs_keyframe_reference_device(h, F->n, st, T, d_ref_slot, out->result, d_work, stream);
    if (rc == HS_OK) rc = hs_keyframe_gate_device(h, d_track_result, prm, out->result, stream);
    if (rc == HS_OK) rc = hs_keyframe_clean_device(h, F->n, st, T, out->result, stream);
    if (rc == HS_OK) rc = hs_keyframe_need_device(h, F->n, F->sensor, d_depth, st, T, K, d_ref_slot, d_track_result, prm, out->result, stream);
    if (rc == HS_OK) rc = hs_keyframe_create_device(h, F, d_depth, d_Tcw, st, T, prm, new_cap, out, d_work, stream);
    if (rc == HS_OK) rc = hs_keyframe_discard_device(h, F->n, st, out->result, stream);
    return rc;
}

}  // extern "C"
