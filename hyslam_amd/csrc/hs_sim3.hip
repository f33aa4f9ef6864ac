// hs_sim3.hip — entry points of the batched Horn Sim3 RANSAC (include/hyslam_amd.h): hs_sim3_plan, hs_sim3_state_init, hs_sim3_work_bytes and
// hs_sim3_iterate(_device) as the two bodies the RANSAC estimators share (hs_ransac.h) over HsSim3Entry.  The kernels are in kernels_sim3.hip.
#include "hs_sim3.h"
#include <algorithm>
#include <cmath>
#include <cstring>

struct HsSim3Entry {
    static constexpr int draw_stride = HS_SIM3_DRAW_STRIDE;
    static constexpr bool mask_inout = false;                     // always written (Sim3Solver.cc:147)
    static constexpr const char* state_init = "hs_sim3_state_init";
    static const char* problem_why(const hs_sim3_params& p) { return p.min_inliers < 0 ? "min_inliers must not be negative" : nullptr; }
    static size_t work_bytes(const HsSim3Args& a) { return HsSim3Work::bytes(a.Q, a.corr_offsets[a.Q], hs_sim3_call_bound(a.Q, a.params, a.corr_offsets, a.n_iterations)); }
    static void launch(const HsSim3Args& a, void* d_work, hipStream_t s) { hs_launch_sim3_iterate(a, d_work, s); }
};

extern "C" {

// SetRansacParameters (Sim3Solver.cc:118-142), expression by expression
int hs_sim3_plan(int N, const hs_sim3_params* params, hs_sim3_plan_t* plan)
{
    if (!params || !plan || N < 0) return HS_ERR_INVALID;
    const float epsilon = (float)params->min_inliers / N;         // int converted to float, divided in float; N = 0 gives an infinity or a NaN
    int nIterations;
    if (params->min_inliers == N) nIterations = 1;
    else {
        const double it = ceil(log(1 - params->probability) / log(1 - pow(epsilon, 3)));
        nIterations = it >= 2147483647.0 ? 2147483647 : it >= 1.0 ? (int)it : 1;            // a NaN or a non-positive count ends as 1, like max(1, .) below
    }
    plan->max_iterations = std::max(1, std::min(nIterations, params->max_iterations));
    plan->epsilon = epsilon;
    return HS_OK;
}

void hs_sim3_state_init(hs_sim3_state* state)
{
    if (state) memset(state, 0, sizeof *state);
}

size_t hs_sim3_work_bytes(int Q, int64_t n_corr_total, int max_hypotheses) { return HsSim3Work::bytes(Q, n_corr_total, max_hypotheses); }

int hs_sim3_iterate_device(hs_orb* h, int Q, const hs_sim3_params* params, const int64_t* corr_offsets, const hs_sim3_corr* d_corrs, int n_iterations,
                           const uint32_t* d_draws, int draw_cap, hs_sim3_state* d_states, uint8_t* d_best_masks, hs_sim3_result* d_results,
                           uint8_t* d_inlier_masks, void* d_work, void* stream)
{
    return hs_ransac_iterate_device<HsSim3Entry>(
        h, HsSim3Args{ Q, params, corr_offsets, d_corrs, n_iterations, d_draws, draw_cap, d_states, d_best_masks, d_results, d_inlier_masks }, d_work, stream);
}

int hs_sim3_iterate(hs_orb* h, int Q, const hs_sim3_params* params, const int64_t* corr_offsets, const hs_sim3_corr* corrs, int n_iterations,
                    const uint32_t* draws, int draw_cap, hs_sim3_state* states, uint8_t* best_masks, hs_sim3_result* results, uint8_t* inlier_masks)
{
    return hs_ransac_iterate_host<HsSim3Entry>(h, HsSim3Args{ Q, params, corr_offsets, corrs, n_iterations, draws, draw_cap, states, best_masks, results, inlier_masks });
}

}  // extern "C"
