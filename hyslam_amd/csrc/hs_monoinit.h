// hs_monoinit.h — monocular initialisation (MonoEstimator, src/initializers/MonoEstimator.cpp): what hs_monoinit.hip (the entry points of
// include/hyslam_amd.h) and kernels_monoinit.hip (the four kernels and their launcher) share.  A problem's N is known only on the device, so the
// planned record holds what the host knows (the two frames, the parameters, D21's constant) and the kernels read N from the work area.
// DESIGN.md 5.21 lists the behaviour item by item.
#pragma once
#include "hs_internal.h"
#include "hs_ransac.h"
#include "hs_work.h"

#define HS_MONO_BATCH 16                // problems per launch group: their planned records travel as kernel arguments
#define HS_MONO_KEY_CHUNK 1024          // key points of each frame k_mono_prepare stages in LDS at a time (x, y of both frames: 16 KB)
#define HS_MONO_CHI_CHUNK 256           // matches whose two chi-squares k_mono_hypotheses keeps in LDS before lane 0 adds them in order (2 KB)
#define HS_MONO_RANK_CHUNK 1024         // cosines k_mono_reconstruct stages in LDS at a time for the rank count (4 KB)
#define HS_MONO_PREP_WORDS 48           // floats per problem k_mono_prepare leaves: T1, T2, T2inv, T2t (9 each), mean and scale of both frames (8), 4 spare
#define HS_MONO_MODEL_WORDS 12          // floats per hypothesis and model in the work area: the 9 of H21 or F21, three spare

// one planned problem, as the kernels read it
struct HsMonoProblem {
    int64_t off1, off2;                 // first key point of frame 1 (also: first match, mask entry, p3d row, work row) and of frame 2
    unsigned long long seed;
    int32_t n1, n2, max_its, min_tri;
    float k[4];                         // fx, fy, cx, cy
    float sigma, min_frac;
    float cos_min_parallax;             // D21: the float nearest cos(min_parallax_deg * pi / 180)
    int32_t q;                          // index into results / draws / the per-problem rows of the work area
};
struct HsMonoBatch { HsMonoProblem p[HS_MONO_BATCH]; };

// the caller's work area, carved for n1: per problem N, the prepared transforms; per key point of frame 1 the compacted match and its cosine; per
// problem, model and hypothesis the score and the model
struct HsMonoWork {
    void* base; int32_t* n /*[Q]*/; float* prep /*[Q * 48]*/; int32_t *m1, *m2 /*[n1_total]*/; float* cosv /*[n1_total]*/; float* score /*[Q * 2 * H]*/;
    float* model /*[Q * 2 * H * 12]*/;
    HsMonoWork(HsWorkCursor& c, int Q, int64_t n1_total, int H) : base(c.here())
    {
        const size_t n1 = n1_total > 0 ? (size_t)n1_total : 0;
        n = c.take<int32_t>(hs_dim(Q)); c.align256();
        prep = c.take<float>(hs_dim(Q) * HS_MONO_PREP_WORDS); c.align256();
        m1 = c.take<int32_t>(n1); c.align256();
        m2 = c.take<int32_t>(n1); c.align256();
        cosv = c.take<float>(n1); c.align256();
        score = c.take<float>(hs_dim(Q) * 2 * hs_dim(H)); c.align256();
        model = c.take<float>(hs_dim(Q) * 2 * hs_dim(H) * HS_MONO_MODEL_WORDS); c.align256();
        c.skip(256);
    }
    static size_t bytes(int Q, int64_t n1_total, int H) { HsWorkCursor c; HsMonoWork(c, Q, n1_total, H); return c.offset(); }
};

// the arguments of hs_monoinit_estimate(_device), host or device pointers by the form, but params and the two offset arrays: always host
struct HsMonoArgs {
    int Q; const hs_monoinit_params* params; const int64_t* key_offsets1; const hs_keypoint* kps1; const int64_t* key_offsets2; const hs_keypoint* kps2;
    const int32_t* matches12; const uint32_t* draws; int draw_cap; hs_monoinit_result* results; uint8_t *inliers_h, *inliers_f; float* p3d; uint8_t* triangulated;
};

// H of a call: the largest max_iterations of its problems (what hs_monoinit_work_bytes' max_iterations has to reach)
int hs_monoinit_call_bound(int Q, const hs_monoinit_params* params);
// enqueues the launch groups of a call on `s`: every pointer of `a` device memory but params and the offsets.  `d_work` is carved for hs_monoinit_call_bound.
void hs_launch_monoinit(const HsMonoArgs& a, void* d_work, hipStream_t s);
