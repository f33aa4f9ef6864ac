// hs_pnp.h — batched EPnP RANSAC (PnPsolver, src/estimators/PnPsolver.cc): what hs_pnp.hip (the entry points of include/hyslam_amd.h) and
// kernels_pnp.hip (the two kernels and their launcher) share.  The plan of a problem is host arithmetic (hs_pnp_plan: glibc's log and pow), so
// the launcher takes the planned problems by value, HS_PNP_BATCH per launch pair, and nothing is copied to the device to describe them.
// DESIGN.md 5.18 lists the behaviour item by item.
#pragma once
#include "hs_internal.h"
#include "hs_ransac.h"
#include "hs_work.h"

#define HS_PNP_BATCH 16                 // problems per launch pair: their planned records travel as kernel arguments

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

using HsPnpArgs = HsRansacArgs<hs_pnp_params, hs_pnp_corr, hs_pnp_state, hs_pnp_result>;

// enqueues the launch pairs of a call on `s`: every pointer of `a` device memory but params and corr_offsets.  `d_work` is carved for hs_pnp_call_bound.
void hs_launch_pnp_iterate(const HsPnpArgs& a, void* d_work, hipStream_t s);
// H of a call: what hs_pnp_work_bytes' max_hypotheses has to reach
int hs_pnp_call_bound(int Q, const hs_pnp_params* params, const int64_t* corr_offsets, int n_iterations);
