// hs_sim3.h — batched Horn Sim3 RANSAC (Sim3Solver, src/estimators/Sim3Solver.cc): what hs_sim3.hip (the entry points of include/hyslam_amd.h) and
// kernels_sim3.hip (the two kernels and their launcher) share.  The plan of a problem is host arithmetic (hs_sim3_plan: glibc's log and pow), so
// the launcher takes the planned problems by value, HS_SIM3_BATCH per launch pair, and nothing is copied to the device to describe them.
// DESIGN.md 5.19 lists the behaviour item by item.
#pragma once
#include "hs_internal.h"
#include "hs_ransac.h"
#include "hs_work.h"

#define HS_SIM3_BATCH 16                // problems per launch pair: their planned records travel as kernel arguments
#define HS_SIM3_CHUNK 256               // correspondences k_sim3_hypotheses stages in LDS at a time (12 floats each: 12 KB)
#define HS_SIM3_POSE_WORDS 16           // floats per hypothesis in the work area: R[9], t[3], s, three spare

// one planned problem, as the kernels read it
struct HsSim3Problem {
    int64_t off;                        // first correspondence
    unsigned long long seed;
    int32_t n, min_inliers, max_its, fix_scale;
    float k1[4], k2[4];                 // fx, fy, cx, cy of the two cameras
    int32_t q;                          // index into states / results / draws
    int32_t _pad;
};
struct HsSim3Batch { HsSim3Problem p[HS_SIM3_BATCH]; };

// the caller's work area: per problem and hypothesis the inlier count and the sixteen floats of R, t and s
struct HsSim3Work {
    void* base; float* hyp_pose /*[Q * H * 16]*/; int32_t* hyp_count /*[Q * H]*/;
    HsSim3Work(HsWorkCursor& c, int Q, int64_t n_total, int H) : base(c.here())
    {
        (void)n_total;                  // nothing is kept per correspondence: the mask of the chosen hypothesis is recomputed from its pose
        hyp_pose = c.take<float>(hs_dim(Q) * hs_dim(H) * HS_SIM3_POSE_WORDS); c.align256();
        hyp_count = c.take<int32_t>(hs_dim(Q) * hs_dim(H)); c.align256();
        c.skip(256);
    }
    static size_t bytes(int Q, int64_t n_total, int H) { HsWorkCursor c; HsSim3Work(c, Q, n_total, H); return c.offset(); }
};

using HsSim3Args = HsRansacArgs<hs_sim3_params, hs_sim3_corr, hs_sim3_state, hs_sim3_result>;

// enqueues the launch pairs of a call on `s`: every pointer of `a` device memory but params and corr_offsets.  `d_work` is carved for hs_sim3_call_bound.
void hs_launch_sim3_iterate(const HsSim3Args& a, void* d_work, hipStream_t s);
// H of a call: what hs_sim3_work_bytes' max_hypotheses has to reach
int hs_sim3_call_bound(int Q, const hs_sim3_params* params, const int64_t* corr_offsets, int n_iterations);
