// hs_stereo.h — the stereo matcher's host interface beyond hs_internal.h: which instance of the matcher a call runs, and the launch functions
// that take the HS_STEREO_KPW knob.  Included after hs_internal.h (kernels_stereo.hip, hs_api.hip), never on its own.
#pragma once

// Left keypoints per wavefront of the matcher launch over `pairs` pairs of `cap` slots: 1 and 2 are k_stereo_match<1> / <2> (every lane walks its
// strip entries AND forms their distances), 4 and 8 are k_stereo_match_compact<K> (the gated candidates of K keypoints queue up in LDS and the
// distances are formed on dense lanes).  knob = HsKnobs::stereo_kpw: 0 = by batch, 1 / 2 / 4 / 8 = that instance whatever the batch (any other
// value counts as 0).  The only place that decides: hs_launch_stereo_kpw and hs_launch_stereo_match_only_kpw both ask here.
int hs_stereo_kpw(int knob, int pairs, int cap);

// hs_launch_stereo / hs_launch_stereo_match_only (hs_internal.h) with the knob; those two mean "by batch" (knob 0)
void hs_launch_stereo_kpw(const hs_keypoint* kpsL, const uint8_t* descL, const int32_t* nL,
                          const hs_keypoint* kpsR, const uint8_t* descR, const int32_t* nR,
                          int pairs, int cap, hs_stereo_params sp, float* uRight, float* depth, int32_t* best_dist,
                          int32_t* strip_count, void* strip_list, int kpw_knob, hipStream_t s);
void hs_launch_stereo_match_only_kpw(const hs_keypoint* kpsL, const uint8_t* descL, const int32_t* nL,
                                     const hs_keypoint* kpsR, const uint8_t* descR, const int32_t* nR,
                                     int pairs, int cap, hs_stereo_params sp, float* uRight, float* depth, int32_t* best_dist,
                                     const int32_t* strip_count, const void* strip_list, int kpw_knob, hipStream_t s);
