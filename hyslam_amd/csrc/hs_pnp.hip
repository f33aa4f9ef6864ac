// hs_pnp.hip — entry points of the batched EPnP RANSAC (include/hyslam_amd.h): hs_pnp_plan, hs_pnp_state_init, hs_pnp_work_bytes and
// hs_pnp_iterate(_device) as the two bodies the RANSAC estimators share (hs_ransac.h) over HsPnpEntry.  The kernels are in kernels_pnp.hip.
#include "hs_pnp.h"
#include <algorithm>
#include <cmath>

struct HsPnpEntry {
    static constexpr int draw_stride = HS_PNP_MAX_SET;
    static constexpr bool mask_inout = true;                      // the mask of a problem that returns no pose comes back as it went
    static constexpr const char* state_init = "hs_pnp_state_init";
    static const char* problem_why(const hs_pnp_params& p) { return p.min_set < 4 || p.min_set > HS_PNP_MAX_SET ? "min_set must lie in [4, HS_PNP_MAX_SET]" : nullptr; }
    static size_t work_bytes(const HsPnpArgs& a) { return HsPnpWork::bytes(a.Q, a.corr_offsets[a.Q], hs_pnp_call_bound(a.Q, a.params, a.corr_offsets, a.n_iterations)); }
    static void launch(const HsPnpArgs& a, void* d_work, hipStream_t s) { hs_launch_pnp_iterate(a, d_work, s); }
};

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
    return hs_ransac_iterate_device<HsPnpEntry>(
        h, HsPnpArgs{ Q, params, corr_offsets, d_corrs, n_iterations, d_draws, draw_cap, d_states, d_best_masks, d_results, d_inlier_masks }, d_work, stream);
}

int hs_pnp_iterate(hs_orb* h, int Q, const hs_pnp_params* params, const int64_t* corr_offsets, const hs_pnp_corr* corrs, int n_iterations,
                   const uint32_t* draws, int draw_cap, hs_pnp_state* states, uint8_t* best_masks, hs_pnp_result* results, uint8_t* inlier_masks)
{
    return hs_ransac_iterate_host<HsPnpEntry>(h, HsPnpArgs{ Q, params, corr_offsets, corrs, n_iterations, draws, draw_cap, states, best_masks, results, inlier_masks });
}

}  // extern "C"
