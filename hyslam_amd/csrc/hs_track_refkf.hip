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
    if (!h) return HS_ERR_INVALID;
    if (!feats_ok(K) || !d_kf_slot || !T || T->L < 0 || (T->L > 0 && !T->lm_bad) || n < 1 || n > 65535 || !d_kps || !d_desc || !d_node || kf_cap < 1 || !d_match_kf ||
        !d_op_view || !d_op_lm || !d_n_matches)
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    hs_launch_search_by_bow_kf(*K, d_kf_slot, *T, d_kps, d_desc, d_node, d_weight, n, th_low, nnratio, d_match_kf, kf_cap, d_op_view, d_op_lm, d_n_matches,
                               hs_stream_or(h, stream));
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_frame_associate_views_device(hs_orb* h, int n, int L, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, const int32_t* d_op_view,
                                    const int32_t* d_op_lm, void* d_work, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (n < 0 || L < 0 || !d_n_matches || !d_work || (n > 0 && (!d_kp_lm || !d_kp_outl || !d_op_view || !d_op_lm))) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    HsWorkCursor c(d_work);
    hs_launch_frame_associate_views(n, L, d_kp_lm, d_kp_outl, d_n_matches, d_op_view, d_op_lm, HsVassocWork(c, n, L), hs_stream_or(h, stream));
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

}  // extern "C"
