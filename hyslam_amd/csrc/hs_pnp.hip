// hs_pnp.hip — entry points of the batched EPnP RANSAC (include/hyslam_amd.h): hs_pnp_plan, hs_pnp_state_init, hs_pnp_work_bytes and
// hs_pnp_iterate(_device).  The kernels and their launcher are in kernels_pnp.hip.  Both forms run the same predicate (hs_pnp_iterate_why) before
// anything is enqueued; the host form stages through HsStage, its work area included, so both forms run the same launches on the same layout.
#include "hs_pnp.h"
#include <algorithm>
#include <cmath>

extern "C" {

// SetRansacParameters (PnPsolver.cc:127-163), expression by expression
int hs_pnp_plan(int N, const hs_pnp_params* params, hs_pnp_plan_t* plan)
{
    if (!params || !plan || N < 0 || params->min_set < 4) return HS_ERR_INVALID;
    float epsilon = params->epsilon;
    const float prod = N * epsilon;                                // int x float, truncated; a product no int holds is clamped, a NaN is 0
    int nMinInliers = prod >= 2147483648.f ? 2147483647 : prod <= -2147483648.f ? -2147483647 - 1 : prod == prod ? (int)prod : 0;
    if (nMinInliers < params->min_inliers) nMinInliers = params->min_inliers;
    if (nMinInliers < params->min_set) nMinInliers = params->min_set;
    if (epsilon < (float)nMinInliers / N) epsilon = (float)nMinInliers / N;
    int nIterations;
    if (nMinInliers == N) nIterations = 1;
    else {
        const double it = ceil(log(1 - params->probability) / log(1 - pow(epsilon, 3)));    // the exponent is 3 although the set is 4
        nIterations = it >= 2147483647.0 ? 2147483647 : it >= 1.0 ? (int)it : 1;            // a NaN or a non-positive count ends as 1, like max(1, .) below
    }
    plan->min_inliers = nMinInliers;
    plan->epsilon = epsilon;
    plan->max_iterations = std::max(1, std::min(nIterations, params->max_iterations));
    plan->_pad = 0;
    return HS_OK;
}

void hs_pnp_state_init(hs_pnp_state* state)
{
    if (!state) return;
    state->iterations = 0; state->best_inliers = 0;
    for (int i = 0; i < 16; i++) state->best_Tcw[i] = 0.f;
}

size_t hs_pnp_work_bytes(int Q, int64_t n_corr_total, int max_hypotheses) { return HsPnpWork::bytes(Q, n_corr_total, max_hypotheses); }

int hs_pnp_iterate_device(hs_orb* h, int Q, const hs_pnp_params* params, const int64_t* corr_offsets, const hs_pnp_corr* d_corrs, int n_iterations,
                          const uint32_t* d_draws, int draw_cap, hs_pnp_state* d_states, uint8_t* d_best_masks, hs_pnp_result* d_results,
                          uint8_t* d_inlier_masks, void* d_work, void* stream)
{
    const char* why = hs_pnp_iterate_why(Q, params, corr_offsets, d_corrs, n_iterations, d_draws, draw_cap, d_states, d_best_masks, d_results, d_inlier_masks, true);
    if (!why && (!d_work || ((uintptr_t)d_work & 15))) why = "d_work is required and 16-byte aligned";
    return hs_device_call(h, why, stream, [&](hipStream_t s) {
        hs_launch_pnp_iterate(Q, params, corr_offsets, d_corrs, n_iterations, d_draws, draw_cap, d_states, d_best_masks, d_results, d_inlier_masks, d_work, s);
    });
}

int hs_pnp_iterate(hs_orb* h, int Q, const hs_pnp_params* params, const int64_t* corr_offsets, const hs_pnp_corr* corrs, int n_iterations,
                   const uint32_t* draws, int draw_cap, hs_pnp_state* states, uint8_t* best_masks, hs_pnp_result* results, uint8_t* inlier_masks)
{
    if (!h) return HS_ERR_INVALID;
    if (const char* why = hs_pnp_iterate_why(Q, params, corr_offsets, corrs, n_iterations, draws, draw_cap, states, best_masks, results, inlier_masks, false))
        return hs_fail(h, HS_ERR_INVALID, why);
    for (int q = 0; q < Q; q++)
        if (states[q].iterations < 0 || states[q].best_inliers < 0) return hs_fail(h, HS_ERR_INVALID, "a state holds a negative count: start from hs_pnp_state_init");
    const size_t n_total = (size_t)corr_offsets[Q];
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    const int H = hs_pnp_call_bound(Q, params, corr_offsets, n_iterations);
    HsStage st(h);
    hs_pnp_corr* d_corrs; uint32_t* d_draws; hs_pnp_state* d_states; uint8_t *d_best, *d_inl, *d_work; hs_pnp_result* d_res;
    st.in(&d_corrs, n_total, corrs);
    st.in(&d_draws, (size_t)Q * (size_t)draw_cap * HS_PNP_MAX_SET, draws);
    st.inout(&d_states, (size_t)Q, states);
    st.inout(&d_best, n_total, best_masks);
    st.out(&d_res, (size_t)Q, results);
    st.inout(&d_inl, n_total, inlier_masks);                       // the mask of a problem that returns no pose comes back as it went
    st.temp(&d_work, HsPnpWork::bytes(Q, (int64_t)n_total, H));
    const int rc = st.begin();
    if (rc != HS_OK) return rc;
    hs_launch_pnp_iterate(Q, params, corr_offsets, d_corrs, n_iterations, draw_cap > 0 ? d_draws : nullptr, draw_cap, d_states, d_best, d_res, d_inl, d_work,
                          st.stream());
    return st.finish();
}

}  // extern "C"
