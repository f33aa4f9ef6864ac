// hs_keyframe.hip — entry points of the stages that follow the two track functions (include/hyslam_amd.h, "after the two track functions"):
// hs_keyframe_reference_device, _gate_, _clean_, _need_, _create_, _discard_ and hs_track_keyframe_device, which is these six in this order: its
// predicate is theirs, on what its enqueue hands them, before the first launch.  Each is the existing stages and the kernels of kernels_keyframe.hip
// enqueued on one stream; nothing here synchronises or reads device memory.
#include "hs_track.h"
#include <cstddef>

namespace {
// the carve of d_work, for a predicate as for an enqueue; the caller's kf_cap is at least T->n_kf (HsKeyframeWork)
HsKeyframeWork work_of(void* d_work, int n, const hs_kf_table* T) { HsWorkCursor c(d_work); return HsKeyframeWork(c, n, T ? T->n_kf : 0); }

// ---- the two stages that are chains themselves (the predicates of the other four are in hs_track.h)
// removeLandMarkAssociation of bad landmarks (:290), then the vote over what is left
const char* reference_why(int n, const hs_track_state* st, const hs_kf_table* T, const int32_t* d_ref_slot, const hs_keyframe_result* d_result, const HsKeyframeWork& w)
{
    if (!kf_n_ok(n) || !state_ok(st) || !T || !d_ref_slot || !d_result || !w.base) return "bad argument";
    return hs_first({ hs_frame_views_why(n, st->kp_lm, st->kp_outl, st->n_matches, T, 1, st->kp_lm_obs),
                      hs_kf_votes_why(T, 1, w.q_off, w.weights, &w.vote[0], &w.vote[1], nullptr, nullptr, 0, &w.vote[2]) });
}
void reference_enqueue(int n, const hs_track_state* st, const hs_kf_table* T, int32_t* d_ref_slot, hs_keyframe_result* d_result, const HsKeyframeWork& w, hipStream_t s)
{
    hs_launch_kfd_ref_begin(n, w.q_off, s);
    hs_launch_frame_views(n, st->kp_lm, st->kp_outl, st->n_matches, *T, 1, st->kp_lm_obs, s);
    hs_kf_votes_enqueue(T, 1, w.q_off, st->kp_lm, nullptr, 1, 0, w.weights, &w.vote[0], &w.vote[1], nullptr, nullptr, 0, &w.vote[2], s);
    hs_launch_kfd_ref_update(&w.vote[0], d_ref_slot, d_result, s);
}
const char* create_why(const hs_frame_view* F, const float* d_depth, const float* d_Tcw, const hs_track_state* st, const hs_kf_table* T, const hs_keyframe_params* prm,
                       int new_cap, const hs_keyframe_out* out, const void* d_work)
{
    if (!F || !kf_n_ok(F->n) || !F->kps || !F->desc || !d_depth || !state_ok(st) || !kf_table_ok(T) || !prm || !keyframe_out_ok(out, new_cap) || !d_work) return "bad argument";
    return hs_pose_views_why(d_Tcw, out->pose_view);
}
void create_enqueue(const hs_frame_view* F, const float* d_depth, const float* d_Tcw, const hs_track_state* st, const hs_kf_table* T, const hs_keyframe_params* prm,
                    int new_cap, const hs_keyframe_out* out, const HsKeyframeWork& w, hipStream_t s)
{
    hs_launch_pose_view(d_Tcw, out->pose_view, nullptr, nullptr, s);                                                   // current_frame.UpdatePoseMatrices() (:32)
    hs_launch_kfd_create(*F, d_depth, *st, *T, *prm, new_cap, *out, w.keys, s);
}
}  // namespace

extern "C" {

size_t hs_keyframe_work_bytes(int n, int kf_cap, int new_cap) { (void)new_cap; return HsKeyframeWork::bytes(n, kf_cap); }

int hs_keyframe_reference_device(hs_orb* h, int n, const hs_track_state* st, const hs_kf_table* T, int32_t* d_ref_slot, hs_keyframe_result* d_result, void* d_work,
                                 void* stream)
{
    const HsKeyframeWork w = work_of(d_work, n, T);
    return hs_device_call(h, reference_why(n, st, T, d_ref_slot, d_result, w), stream, [&](hipStream_t s) { reference_enqueue(n, st, T, d_ref_slot, d_result, w, s); });
}

int hs_keyframe_gate_device(hs_orb* h, const hs_track_result* d_track_result, const hs_keyframe_params* prm, hs_keyframe_result* d_result, void* stream)
{
    return hs_device_call(h, hs_keyframe_gate_why(d_track_result, prm, d_result), stream, [&](hipStream_t s) { hs_launch_kfd_gate(d_track_result, *prm, d_result, s); });
}

int hs_keyframe_clean_device(hs_orb* h, int n, const hs_track_state* st, const hs_kf_table* T, hs_keyframe_result* d_result, void* stream)
{
    return hs_device_call(h, hs_keyframe_clean_why(n, st, T, d_result), stream, [&](hipStream_t s) { hs_launch_kfd_clean(n, *st, *T, d_result, s); });
}

int hs_keyframe_need_device(hs_orb* h, int n, int sensor, const float* d_depth, const hs_track_state* st, const hs_kf_table* T, const hs_kf_features* K,
                            const int32_t* d_ref_slot, const hs_track_result* d_track_result, const hs_keyframe_params* prm, hs_keyframe_result* d_result, void* stream)
{
    return hs_device_call(h, hs_keyframe_need_why(n, sensor, d_depth, st, T, K, d_ref_slot, prm, d_result), stream,
                          [&](hipStream_t s) { hs_launch_kfd_need(n, sensor, d_depth, *st, *T, *K, d_ref_slot, d_track_result, *prm, d_result, s); });
}

int hs_keyframe_create_device(hs_orb* h, const hs_frame_view* F, const float* d_depth, const float* d_Tcw, const hs_track_state* st, const hs_kf_table* T,
                              const hs_keyframe_params* prm, int new_cap, const hs_keyframe_out* out, void* d_work, void* stream)
{
    return hs_device_call(h, create_why(F, d_depth, d_Tcw, st, T, prm, new_cap, out, d_work), stream,
                          [&](hipStream_t s) { create_enqueue(F, d_depth, d_Tcw, st, T, prm, new_cap, out, work_of(d_work, F->n, T), s); });
}

int hs_keyframe_discard_device(hs_orb* h, int n, const hs_track_state* st, hs_keyframe_result* d_result, void* stream)
{
    return hs_device_call(h, hs_keyframe_discard_why(n, st, d_result), stream, [&](hipStream_t s) { hs_launch_kfd_discard(n, *st, d_result, s); });
}

int hs_track_keyframe_device(hs_orb* h, const hs_frame_view* F, const float* d_depth, const float* d_Tcw, const hs_kf_table* T, const hs_kf_features* K,
                             const hs_track_result* d_track_result, const hs_keyframe_params* prm, const hs_track_state* st, int32_t* d_ref_slot, int new_cap,
                             const hs_keyframe_out* out, void* d_work, void* stream)
{
    const int n = F ? F->n : 0;
    const HsKeyframeWork w = work_of(d_work, n, T);
    hs_keyframe_result* res = out ? out->result : nullptr;
    const char* why = hs_bad(!F || !out);
    if (!why) why = hs_first({ reference_why(n, st, T, d_ref_slot, res, w), hs_keyframe_gate_why(d_track_result, prm, res), hs_keyframe_clean_why(n, st, T, res),
                               hs_keyframe_need_why(n, F->sensor, d_depth, st, T, K, d_ref_slot, prm, res), create_why(F, d_depth, d_Tcw, st, T, prm, new_cap, out, d_work),
                               hs_keyframe_discard_why(n, st, res) });
    return hs_device_call(h, why, stream, [&](hipStream_t s) {
        reference_enqueue(n, st, T, d_ref_slot, res, w, s);
        hs_launch_kfd_gate(d_track_result, *prm, res, s);
        hs_launch_kfd_clean(n, *st, *T, res, s);
        hs_launch_kfd_need(n, F->sensor, d_depth, *st, *T, *K, d_ref_slot, d_track_result, *prm, res, s);
        create_enqueue(F, d_depth, d_Tcw, st, T, prm, new_cap, out, w, s);
        hs_launch_kfd_discard(n, *st, res, s);
    });
}

}  // extern "C"
