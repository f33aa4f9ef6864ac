// hs_track_refkf.hip — entry points of the two steps of TrackReferenceKeyFrame::track that had no resident form (include/hyslam_amd.h):
// hs_search_by_bow_kf_device and hs_frame_associate_views_device.  Launches of kernels_track_refkf.hip on one stream; nothing here synchronises,
// reads device memory or claims the handle's scratch.
#include "hs_track.h"
#include <cstddef>

extern "C" {

size_t hs_track_refkf_work_bytes(int n, int kf_cap, int L) { (void)kf_cap; return HsVassocWork::bytes(n, L); }

int hs_search_by_bow_kf_device(hs_orb* h, const hs_kf_features* K, const int32_t* d_kf_slot, const hs_kf_table* T, const hs_keypoint* d_kps, const uint8_t* d_desc,
                               const int32_t* d_node, const float* d_weight, int n, float th_low, float nnratio, int32_t* d_match_kf, int kf_cap, int32_t* d_op_view,
                               int32_t* d_op_lm, int32_t* d_n_matches, void* d_work, void* stream)
{
    (void)d_work;
    return hs_device_call(h, hs_search_by_bow_kf_why(K, d_kf_slot, T, d_kps, d_desc, d_node, n, d_match_kf, kf_cap, d_op_view, d_op_lm, d_n_matches), stream,
                          [&](hipStream_t s) {
        hs_launch_search_by_bow_kf(*K, d_kf_slot, *T, d_kps, d_desc, d_node, d_weight, n, th_low, nnratio, d_match_kf, kf_cap, d_op_view, d_op_lm, d_n_matches, s);
    });
}

int hs_frame_associate_views_device(hs_orb* h, int n, int L, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, const int32_t* d_op_view,
                                    const int32_t* d_op_lm, void* d_work, void* stream)
{
    return hs_device_call(h, hs_frame_associate_views_why(n, L, d_kp_lm, d_kp_outl, d_n_matches, d_op_view, d_op_lm, d_work), stream, [&](hipStream_t s) {
        HsWorkCursor c(d_work);
        hs_launch_frame_associate_views(n, L, d_kp_lm, d_kp_outl, d_n_matches, d_op_view, d_op_lm, HsVassocWork(c, n, L), s);
    });
}

}  // extern "C"
