// hs_sim3.hip — entry points of the batched Horn Sim3 RANSAC (include/hyslam_amd.h): hs_sim3_plan, hs_sim3_state_init, hs_sim3_work_bytes and
// hs_sim3_iterate(_device).  The kernels and their launcher are in kernels_sim3.hip.  Both forms run the same predicate (hs_sim3_iterate_why) before
// anything is enqueued; the host form stages through HsStage, its work area included, so both forms run the same launches on the same layout.
#include "hs_sim3.h"
#include <algorithm>
#include <cmath>
#include <cstring>

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
    const char* why = hs_sim3_iterate_why(Q, params, corr_offsets, d_corrs, n_iterations, d_draws, draw_cap, d_states, d_best_masks, d_results, d_inlier_masks, true);
    if (!why && (!d_work || ((uintptr_t)d_work & 15))) why = "d_work is required and 16-byte aligned";
    return hs_device_call(h, why, stream, [&](hipStream_t s) {
        hs_launch_sim3_iterate(Q, params, corr_offsets, d_corrs, n_iterations, d_draws, draw_cap, d_states, d_best_masks, d_results, d_inlier_masks, d_work, s);
    });
}

int hs_sim3_iterate(hs_orb* h, int Q, const hs_sim3_params* params, const int64_t* corr_offsets, const hs_sim3_corr* corrs, int n_iterations,
                    const uint32_t* draws, int draw_cap, hs_sim3_state* states, uint8_t* best_masks, hs_sim3_result* results, uint8_t* inlier_masks)
{
    if (!h) return HS_ERR_INVALID;
    if (const char* why = hs_sim3_iterate_why(Q, params, corr_offsets, corrs, n_iterations, draws, draw_cap, states, best_masks, results, inlier_masks, false))
        return hs_fail(h, HS_ERR_INVALID, why);
    for (int q = 0; q < Q; q++)
        if (states[q].iterations < 0 || states[q].best_inliers < 0) return hs_fail(h, HS_ERR_INVALID, "a state holds a negative count: start from hs_sim3_state_init");
    const size_t n_total = (size_t)corr_offsets[Q];
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    const int H = hs_sim3_call_bound(Q, params, corr_offsets, n_iterations);
    HsStage st(h);
    hs_sim3_corr* d_corrs; uint32_t* d_draws; hs_sim3_state* d_states; uint8_t *d_best, *d_inl, *d_work; hs_sim3_result* d_res;
    st.in(&d_corrs, n_total, corrs);
    st.in(&d_draws, (size_t)Q * (size_t)draw_cap * HS_SIM3_DRAW_STRIDE, draws);
    st.inout(&d_states, (size_t)Q, states);
    st.inout(&d_best, n_total, best_masks);
    st.out(&d_res, (size_t)Q, results);
    st.out(&d_inl, n_total, inlier_masks);                         // always written (Sim3Solver.cc:147)
    st.temp(&d_work, HsSim3Work::bytes(Q, (int64_t)n_total, H));
    const int rc = st.begin();
    if (rc != HS_OK) return rc;
    hs_launch_sim3_iterate(Q, params, corr_offsets, d_corrs, n_iterations, draw_cap > 0 ? d_draws : nullptr, draw_cap, d_states, d_best, d_res, d_inl, d_work,
                           st.stream());
    return st.finish();
}

}  // extern "C"
