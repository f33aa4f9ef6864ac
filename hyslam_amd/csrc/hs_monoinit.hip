// hs_monoinit.hip — entry points of the monocular initialisation (include/hyslam_amd.h): hs_monoinit_work_bytes, hs_monoinit_check and
// hs_monoinit_estimate(_device).  The call keeps no state between calls, so it is not an HsRansacArgs / hs_ransac_iterate_* user (hs_ransac.h): it takes
// from that layer what fits as it is — the draws, the sampler, the launcher's batching — and follows its split of check from enqueue.  The kernels
// are in kernels_monoinit.hip.
#include "hs_monoinit.h"
#include <cmath>

static const char* hs_monoinit_why(const HsMonoArgs& a, bool device, const void* d_work)
{
    if (a.Q < 1 || !a.params || !a.key_offsets1 || !a.key_offsets2 || !a.results) return "bad argument";
    if (a.draw_cap < 0 || (a.draw_cap > 0 && !a.draws)) return "bad argument";
    if (!hs_csr_ok(a.key_offsets1, a.Q) || !hs_csr_ok(a.key_offsets2, a.Q)) return "offsets must be non-negative and non-decreasing";
    if (a.key_offsets1[a.Q] > 0 && (!a.kps1 || !a.matches12 || !a.inliers_h || !a.inliers_f || !a.p3d || !a.triangulated)) return "bad argument";
    if (a.key_offsets2[a.Q] > 0 && !a.kps2) return "bad argument";
    for (int q = 0; q < a.Q; q++) {
        const hs_monoinit_params& p = a.params[q];
        if (a.key_offsets1[q + 1] - a.key_offsets1[q] > 0x7fffffff || a.key_offsets2[q + 1] - a.key_offsets2[q] > 0x7fffffff) return "a frame holds at most 2^31 - 1 key points";
        if (p.max_iterations < 1 || p.max_iterations > HS_MONOINIT_MAX_ITERATIONS) return "max_iterations must lie in [1, HS_MONOINIT_MAX_ITERATIONS]";
        if (!(p.sigma > 0.f) || !std::isfinite(p.sigma)) return "sigma must be positive and finite";
        if (!(p.fx > 0.f) || !(p.fy > 0.f) || !std::isfinite(p.fx) || !std::isfinite(p.fy) || !std::isfinite(p.cx) || !std::isfinite(p.cy)) return "the camera must be finite with positive focal lengths";
        if (!(p.min_parallax_deg > 0.f) || !(p.min_parallax_deg < 180.f)) return "min_parallax_deg must lie in (0, 180)";
        if (!std::isfinite(p.min_frac_triangulated)) return "min_frac_triangulated must be finite";
        if (p.min_triangulated < 0) return "min_triangulated must not be negative";
    }
    if (device && (((uintptr_t)a.kps1 & 15) || ((uintptr_t)a.kps2 & 15))) return "d_kps1 and d_kps2 are 16-byte aligned";
    if (device && (!d_work || ((uintptr_t)d_work & 15))) return "d_work is required and 16-byte aligned";
    return nullptr;
}

extern "C" {

size_t hs_monoinit_work_bytes(int Q, int64_t n1_total, int max_iterations) { return HsMonoWork::bytes(Q, n1_total, max_iterations); }

const char* hs_monoinit_check(int Q, const hs_monoinit_params* params, const int64_t* key_offsets1, const hs_keypoint* kps1, const int64_t* key_offsets2,
                              const hs_keypoint* kps2, const int32_t* matches12, const uint32_t* draws, int draw_cap, const hs_monoinit_result* results,
                              const uint8_t* inliers_h, const uint8_t* inliers_f, const float* p3d, const uint8_t* triangulated, int device, const void* d_work)
{
    return hs_monoinit_why(HsMonoArgs{ Q, params, key_offsets1, kps1, key_offsets2, kps2, matches12, draws, draw_cap, const_cast<hs_monoinit_result*>(results),
                                       const_cast<uint8_t*>(inliers_h), const_cast<uint8_t*>(inliers_f), const_cast<float*>(p3d), const_cast<uint8_t*>(triangulated) },
                           device != 0, d_work);
}

int hs_monoinit_estimate_device(hs_orb* h, int Q, const hs_monoinit_params* params, const int64_t* key_offsets1, const hs_keypoint* d_kps1,
                                const int64_t* key_offsets2, const hs_keypoint* d_kps2, const int32_t* d_matches12, const uint32_t* d_draws, int draw_cap,
                                hs_monoinit_result* d_results, uint8_t* d_inliers_h, uint8_t* d_inliers_f, float* d_p3d, uint8_t* d_triangulated, void* d_work,
                                void* stream)
{
    const HsMonoArgs a{ Q, params, key_offsets1, d_kps1, key_offsets2, d_kps2, d_matches12, draw_cap > 0 ? d_draws : nullptr, draw_cap, d_results, d_inliers_h, d_inliers_f,
                        d_p3d, d_triangulated };
    return hs_device_call(h, hs_monoinit_why(a, true, d_work), stream, [&](hipStream_t s) { hs_launch_monoinit(a, d_work, s); });
}

int hs_monoinit_estimate(hs_orb* h, int Q, const hs_monoinit_params* params, const int64_t* key_offsets1, const hs_keypoint* kps1, const int64_t* key_offsets2,
                         const hs_keypoint* kps2, const int32_t* matches12, const uint32_t* draws, int draw_cap, hs_monoinit_result* results, uint8_t* inliers_h,
                         uint8_t* inliers_f, float* p3d, uint8_t* triangulated)
{
    if (!h) return HS_ERR_INVALID;
    const HsMonoArgs a{ Q, params, key_offsets1, kps1, key_offsets2, kps2, matches12, draws, draw_cap, results, inliers_h, inliers_f, p3d, triangulated };
    if (const char* why = hs_monoinit_why(a, false, nullptr)) return hs_fail(h, HS_ERR_INVALID, why);
    const size_t n1 = (size_t)key_offsets1[Q], n2 = (size_t)key_offsets2[Q];
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    HsStage st(h);
    hs_keypoint *d_k1, *d_k2; int32_t* d_m; uint32_t* d_draws; hs_monoinit_result* d_res; uint8_t *d_ih, *d_if, *d_tri, *d_work; float* d_p3d;
    st.in(&d_k1, n1, kps1);
    st.in(&d_k2, n2, kps2);
    st.in(&d_m, n1, matches12);
    st.in(&d_draws, (size_t)Q * (size_t)draw_cap * HS_MONOINIT_DRAW_STRIDE, draws);
    st.out(&d_res, (size_t)Q, results);
    st.out(&d_ih, n1, inliers_h);
    st.out(&d_if, n1, inliers_f);
    st.out(&d_p3d, n1 * 3, p3d);
    st.out(&d_tri, n1, triangulated);
    st.temp(&d_work, HsMonoWork::bytes(Q, key_offsets1[Q], hs_monoinit_call_bound(Q, params)));
    const int rc = st.begin();
    if (rc != HS_OK) return rc;
    hs_launch_monoinit(HsMonoArgs{ Q, params, key_offsets1, d_k1, key_offsets2, d_k2, d_m, draw_cap > 0 ? d_draws : nullptr, draw_cap, d_res, d_ih, d_if, d_p3d, d_tri },
                       d_work, st.stream());
    return st.finish();
}

}  // extern "C"
