// hs_track_initial.hip — TrackingStateNormal::initialPoseEstimation as one enqueue-only call (include/hyslam_amd.h, "initial pose estimation as one
// resident call"): hs_track_reference_keyframe_device, hs_track_initial_device and hs_track_normal_device.  Each is the existing stages and the gate
// kernels of kernels_track_initial.hip enqueued on one stream; its predicate is its stages' predicates (hs_track.h) on what its enqueue hands them, all
// of them before the first launch; nothing here synchronises, reads device memory or claims the handle's scratch (the motion and local stages'
// projection searches take their grid lists).
#include "hs_track.h"
#include <cstddef>

namespace {
bool iout_ok(const hs_track_initial_out* o, bool frame_result)
{
    return o && o->bow_word && o->bow_weight && o->bow_node && o->match_kf && o->op_view && o->op_lm && o->pose_view && o->problem && o->edges && o->outlier &&
           o->n_edges && o->pose && o->Tcw_init && o->result && (!frame_result || o->frame_result) && !((uintptr_t)o->edges & 15);
}
// the arguments the three calls share and what the stages derive from them: formed once, read by the predicates and by the enqueues
struct Refkf {
    HsTrackPlan t;                                               // F, T, d_lms, tp, st, Fs; its carve is the motion and local stages': HsTrackWork heads the area
    const hs_vocab_dev* vocab; const hs_kf_features* K; const int32_t* d_kf_slot; int kf_cap; const float* d_Tcw_last; const hs_track_refkf_params* rp;
    const hs_track_initial_out* o;
    HsWorkCursor c; HsInitialWork w;
    Refkf(const hs_frame_view* F, const hs_vocab_dev* vocab, const hs_kf_features* K, const int32_t* d_kf_slot, int kf_cap, const float* d_Tcw_last, const hs_kf_table* T,
          const hs_landmark* d_lms, const hs_track_params* tp, const hs_track_refkf_params* rp, const hs_track_state* st, const hs_track_out* out,
          const hs_track_initial_out* o, void* d_work)
        : t(F, T, d_lms, tp, st, out, d_work), vocab(vocab), K(K), d_kf_slot(d_kf_slot), kf_cap(kf_cap), d_Tcw_last(d_Tcw_last), rp(rp), o(o), c(t.ok ? d_work : nullptr),
          w(c, t.Fs.n, t.ok ? T->L : 0) {}
    HsPoseTail tail() const { return HsPoseTail{ HS_TRACK_MOTION, o->problem, o->edges, o->outlier, o->pose, o->n_edges, nullptr, o->result, &o->result->n_matches_map_refkf }; }
};
// the motion stage's own arguments
struct Motion { const float* d_Tcw_pred; const hs_keypoint* d_last_kps; const int32_t* d_last_kp_lm; int n_last; };

// d_Tcw_entry: the pose the stage restores where it is skipped
const char* refkf_why(const Refkf& a, int device, const float* d_Tcw_entry, bool frame_result)
{
    // the structs, and what the glue kernels read that are no entry point of their own (k_init_gate, k_init_edges_gate, k_init_finish)
    const HsTrackPlan& t = a.t;
    if (!t.ok || !a.rp || t.T->L < 1 || !t.d_lms || ((uintptr_t)t.d_lms & 15) || !state_ok(t.st) || !iout_ok(a.o, frame_result) || !d_Tcw_entry) return "bad argument";
    const hs_frame_view* F = t.F; const hs_track_state* st = t.st; const hs_track_initial_out* o = a.o;
    return hs_first({ hs_bow_transform_why(a.vocab, device, F->desc, F->n, o->bow_word, o->bow_weight, o->bow_node),
                      hs_search_by_bow_kf_why(a.K, a.d_kf_slot, t.T, F->kps, F->desc, o->bow_node, F->n, o->match_kf, a.kf_cap, o->op_view, o->op_lm, &o->result->n_bow),
                      hs_frame_associate_views_why(F->n, t.T->L, st->kp_lm, st->kp_outl, st->n_matches, a.w.op_view_run, a.w.op_lm_run, a.w.vassoc.base),
                      hs_pose_views_why(a.d_Tcw_last, o->pose_view), hs_pose_tail_why(a.tail(), t) });
}
// d_motion (may be nullptr): the motion stage's result the stage is predicated on
void refkf_enqueue(const Refkf& a, const float* d_Tcw_entry, const hs_track_result* d_motion, hipStream_t s)
{
    const hs_frame_view* F = a.t.F; const hs_track_state* st = a.t.st; const hs_track_initial_out* o = a.o;
    const int n = F->n, L = a.t.T->L;
    hs_bow_transform_enqueue(a.vocab, F->desc, nullptr, n, o->bow_word, o->bow_weight, o->bow_node, s);                                   // Frame::ComputeBoW
    hs_launch_search_by_bow_kf(*a.K, a.d_kf_slot, *a.t.T, F->kps, F->desc, o->bow_node, o->bow_weight, n, a.rp->th_low, a.rp->nnratio, o->match_kf, a.kf_cap, o->op_view,
                               o->op_lm, &o->result->n_bow, s);
    hs_launch_init_gate(n, d_motion, *a.rp, o->op_view, o->op_lm, a.w.op_view_run, a.w.op_lm_run, o->result, s);      // both `if`s, as one status
    hs_launch_frame_associate_views(n, L, st->kp_lm, st->kp_outl, st->n_matches, a.w.op_view_run, a.w.op_lm_run, a.w.vassoc, s);          // associateLandMarks
    hs_launch_pose_view(a.d_Tcw_last, o->pose_view, o->problem, F, s);                                                                    // SetPose(last_frame.mTcw)
    hs_pose_tail_enqueue(a.tail(), a.t, s);
    hs_launch_init_finish(d_motion, a.rp->thresh_init, o->pose, d_Tcw_entry, o->Tcw_init, o->result, s);
}

// initialPoseEstimation: the motion stage where the velocity is valid (without one its arguments are not read), then the reference key frame
const char* initial_why(const Refkf& a, int device, int velocity_valid, const Motion& m, const float* d_Tcw_entry, bool frame_result)
{
    if (!velocity_valid) return refkf_why(a, device, d_Tcw_entry, frame_result);
    const char* why = hs_track_motion_why(a.t, m.d_Tcw_pred, m.d_last_kps, m.d_last_kp_lm, m.n_last);
    return why ? why : refkf_why(a, device, a.t.out->pose_motion->Tcw, frame_result);
}
int initial_enqueue(hs_orb* h, const Refkf& a, int velocity_valid, const Motion& m, const float* d_Tcw_entry, hipStream_t s)
{
    if (!velocity_valid) { refkf_enqueue(a, d_Tcw_entry, nullptr, s); return HS_OK; }
    const int rc = hs_track_motion_enqueue(h, a.t, m.d_Tcw_pred, m.d_last_kps, m.d_last_kp_lm, m.n_last, s);
    if (rc == HS_OK) refkf_enqueue(a, a.t.out->pose_motion->Tcw, a.t.out->result, s);
    return rc;
}
}  // namespace

extern "C" {

size_t hs_track_initial_work_bytes(int n, int n_last, int L, int cap, int kf_cap) { (void)n_last; (void)cap; (void)kf_cap; return HsInitialWork::bytes(n, L); }

int hs_track_reference_keyframe_device(hs_orb* h, const hs_frame_view* F, const hs_vocab_dev* vocab, const hs_kf_features* K, const int32_t* d_kf_slot, int kf_cap,
                                       const float* d_Tcw_last, const float* d_Tcw_entry, const hs_track_result* d_motion_result, const hs_kf_table* T,
                                       const hs_landmark* d_lms, const hs_track_params* tp, const hs_track_refkf_params* rp, const hs_track_state* st,
                                       const hs_track_initial_out* iout, void* d_work, void* stream)
{
    const Refkf a(F, vocab, K, d_kf_slot, kf_cap, d_Tcw_last, T, d_lms, tp, rp, st, nullptr, iout, d_work);
    return hs_device_call(h, refkf_why(a, hs_orb_device_of(h), d_Tcw_entry, false), stream, [&](hipStream_t s) { refkf_enqueue(a, d_Tcw_entry, d_motion_result, s); });
}

int hs_track_initial_device(hs_orb* h, const hs_frame_view* F, int velocity_valid, const float* d_Tcw_pred, const hs_keypoint* d_last_kps, const int32_t* d_last_kp_lm,
                            int n_last, const hs_vocab_dev* vocab, const hs_kf_features* K, const int32_t* d_kf_slot, int kf_cap, const float* d_Tcw_last,
                            const float* d_Tcw_entry, const hs_kf_table* T, const hs_landmark* d_lms, const hs_track_params* tp, const hs_track_refkf_params* rp,
                            const hs_track_state* st, const hs_track_out* out, const hs_track_initial_out* iout, void* d_work, void* stream)
{
    const Refkf a(F, vocab, K, d_kf_slot, kf_cap, d_Tcw_last, T, d_lms, tp, rp, st, out, iout, d_work);
    const Motion m{ d_Tcw_pred, d_last_kps, d_last_kp_lm, n_last };
    return hs_device_call(h, initial_why(a, hs_orb_device_of(h), velocity_valid, m, d_Tcw_entry, false), stream,
                          [&](hipStream_t s) { return initial_enqueue(h, a, velocity_valid, m, d_Tcw_entry, s); });
}

int hs_track_normal_device(hs_orb* h, const hs_frame_view* F, int velocity_valid, const float* d_Tcw_pred, const hs_keypoint* d_last_kps, const int32_t* d_last_kp_lm,
                           int n_last, const hs_vocab_dev* vocab, const hs_kf_features* K, const int32_t* d_kf_slot, int kf_cap, const float* d_Tcw_last,
                           const float* d_Tcw_entry, const hs_kf_table* T, const hs_landmark* d_lms, const int32_t* d_neigh, int neigh_cap, const int32_t* d_parent, int cap,
                           const hs_track_params* tp, const hs_track_refkf_params* rp, const hs_track_state* st, const hs_track_out* out,
                           const hs_track_initial_out* iout, void* d_work, void* stream)
{
    const Refkf a(F, vocab, K, d_kf_slot, kf_cap, d_Tcw_last, T, d_lms, tp, rp, st, out, iout, d_work);
    const Motion m{ d_Tcw_pred, d_last_kps, d_last_kp_lm, n_last };
    const char* why = initial_why(a, hs_orb_device_of(h), velocity_valid, m, d_Tcw_entry, true);
    if (!why) why = hs_track_local_why(a.t, iout->Tcw_init, d_neigh, neigh_cap, d_parent, cap);
    if (!why) why = hs_bad(iout->frame_result == out->result);   // k_frame_result reads the stages' record while it writes the frame's
    return hs_device_call(h, why, stream, [&](hipStream_t s) {
        int rc = initial_enqueue(h, a, velocity_valid, m, d_Tcw_entry, s);
        if (rc == HS_OK) rc = hs_track_local_enqueue(h, a.t, iout->Tcw_init, d_neigh, neigh_cap, d_parent, cap, s);
        if (rc == HS_OK) hs_launch_frame_result(velocity_valid ? out->result : nullptr, iout->result, &out->result->n_inliers, iout->frame_result, s);
        return rc;
    });
}

}  // extern "C"
