// hs_pnp.h — batched EPnP RANSAC (PnPsolver, src/estimators/PnPsolver.cc): what hs_pnp.hip (the entry points of include/hyslam_amd.h) and
// kernels_pnp.hip (the two kernels and their launcher) share.  The plan of a problem is host arithmetic (hs_pnp_plan: glibc's log and pow), so
// the launcher takes the planned problems by value, HS_PNP_BATCH per launch pair, and nothing is copied to the device to describe them.
// DESIGN.md 5.18 lists the behaviour item by item.
#pragma once
#include "hs_internal.h"
#include "hs_work.h"

#define HS_PNP_BATCH 16                 // problems per launch pair: their planned records travel as kernel arguments
#define HS_PNP_SVD_SWEEPS 30            // cap on the sweeps of the one-sided Jacobi SVD

// one planned problem, as the kernels read it
struct HsPnpProblem {
    int64_t off;                        // first correspondence
    unsigned long long seed;
    int32_t n, min_inliers, max_its, min_set;   // N and the three effective values of hs_pnp_plan
    float th2, fx, fy, cx, cy;
    int32_t q;                          // index into states / results / draws
};
struct HsPnpBatch { HsPnpProblem p[HS_PNP_BATCH]; };

// the caller's work area: per problem and hypothesis the inlier count and the twelve doubles of R and t, per correspondence the refine's
// compacted points (five doubles) and the mask of the refine's recount
struct HsPnpWork {
    void* base; double* hyp_pose /*[Q * H * 12]*/; double* pts /*[n_total * 5]*/; int32_t* hyp_count /*[Q * H]*/; uint8_t* tmp_mask /*[n_total]*/;
    HsPnpWork(HsWorkCursor& c, int Q, int64_t n_total, int H) : base(c.here())
    {
        const size_t nt = n_total > 0 ? (size_t)n_total : 0;
        hyp_pose = c.take<double>(hs_dim(Q) * hs_dim(H) * 12); c.align256();
        pts = c.take<double>(nt * 5); c.align256();
        hyp_count = c.take<int32_t>(hs_dim(Q) * hs_dim(H)); c.align256();
        tmp_mask = c.take<uint8_t>(nt); c.align256();
        c.skip(256);
    }
    static size_t bytes(int Q, int64_t n_total, int H) { HsWorkCursor c; HsPnpWork(c, Q, n_total, H); return c.offset(); }
};

// hypotheses a call of `n_iterations` runs at most for a problem planned to `max_its`: the loop's OR (PnPsolver.cc:188)
inline int hs_pnp_bound(int max_its, int n_iterations) { return max_its > n_iterations ? max_its : n_iterations; }

// the predicate both forms share: pure host code over the by-value arguments and the two host arrays
inline const char* hs_pnp_iterate_why(int Q, const hs_pnp_params* params, const int64_t* corr_offsets, const hs_pnp_corr* corrs, int n_iterations,
                                      const uint32_t* draws, int draw_cap, const hs_pnp_state* states, const uint8_t* best_masks, const hs_pnp_result* results,
                                      const uint8_t* inlier_masks, bool device)
{
    if (Q < 1 || !params || !corr_offsets || !states || !results) return "bad argument";
    if (n_iterations < 1) return "n_iterations must be positive";
    if (draw_cap < 0 || (draw_cap > 0 && !draws)) return "bad argument";
    if (!hs_csr_ok(corr_offsets, Q)) return "offsets must be non-negative and non-decreasing";
    if (corr_offsets[Q] > 0 && (!corrs || !best_masks || !inlier_masks)) return "bad argument";
    if (device && ((uintptr_t)corrs & 15)) return "d_corrs is 16-byte aligned";
    for (int q = 0; q < Q; q++) {
        if (params[q].min_set < 4 || params[q].min_set > HS_PNP_MAX_SET) return "min_set must lie in [4, HS_PNP_MAX_SET]";
        if (corr_offsets[q + 1] - corr_offsets[q] > 0x7fffffff) return "a problem holds at most 2^31 - 1 correspondences";
    }
    return nullptr;
}

// all pointers device memory but params and corr_offsets; asynchronous on `s`.  `work` is carved for H = the largest hs_pnp_bound of the call.
void hs_launch_pnp_iterate(int Q, const hs_pnp_params* params, const int64_t* corr_offsets, const hs_pnp_corr* d_corrs, int n_iterations, const uint32_t* d_draws,
                           int draw_cap, hs_pnp_state* d_states, uint8_t* d_best_masks, hs_pnp_result* d_results, uint8_t* d_inlier_masks, void* d_work, hipStream_t s);
// H of a call: what hs_pnp_work_bytes' max_hypotheses has to reach
int hs_pnp_call_bound(int Q, const hs_pnp_params* params, const int64_t* corr_offsets, int n_iterations);
