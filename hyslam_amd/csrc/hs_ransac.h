// hs_ransac.h — what the two RANSAC estimators (hs_pnp.*, kernels_pnp.hip: PnPsolver; hs_sim3.*, kernels_sim3.hip: Sim3Solver) share, stated once
// (DESIGN.md 5.20): the draws of D18, the sampler with its two write policies, the two loop rules, a launcher's batching, the predicate of a call and
// the bodies of its two forms.  The device side is plain __host__ __device__ inline code: a host build of a kernel file computes the same bits.
#pragma once
#include "hs_internal.h"
#include <climits>

#define HS_RANSAC_HD __host__ __device__

// SplitMix64's finaliser on counter c
HS_RANSAC_HD inline unsigned long long hs_ransac_mix(unsigned long long c)
{
    unsigned long long z = 0x9E3779B97F4A7C15ull * (c + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the 32-bit word that draw k of absolute iteration `it` of problem q reduces: row `it` of the problem's directed table (`stride` words a row) while
// 0 <= it < draw_cap, else the generator's word on the counter seed + it * set + k
HS_RANSAC_HD inline unsigned int hs_ransac_draw(const uint32_t* draws, int draw_cap, int stride, int q, unsigned long long seed, long long it, int set, int k)
{
    return it >= 0 && it < draw_cap ? draws[((size_t)q * (size_t)draw_cap + (size_t)it) * stride + k]
                                    : (unsigned int)(hs_ransac_mix(seed + (unsigned long long)it * (unsigned long long)set + (unsigned long long)k) >> 32);
}

// The sample of absolute iteration `it` of the planned problem p (its n, q and seed): `set` <= MAX_SET draws out of avail = 0 .. n-1,
// randi = (word * avail) >> 32 < avail.  Every draw takes idx = avail[randi], writes the back element somewhere and pops; WHERE is the one
// difference between the two solvers:
//   WRITE_AT_VALUE = false   PnPsolver.cc:194-207: avail[randi] = avail.back() — swap-with-back, no index is drawn twice
//   WRITE_AT_VALUE = true    Sim3Solver.cc:167-181: avail[idx] = avail.back() — the place named by the VALUE drawn; a write to a place that was popped
//                            already has no effect, and an index can be drawn twice.  Reference behaviour, kept.
// Only the places a draw wrote differ from their index, so at most `set` of them are kept (pos, val).  n >= set, so avail >= 1 at every draw.
// `set` is a reference so that a set size kept in the problem record (PnP's min_set, a kernel argument) is read where it lies, not copied.
template <int MAX_SET, bool WRITE_AT_VALUE, class P>
HS_RANSAC_HD inline void hs_ransac_sample(const P& p, const int& set, const uint32_t* draws, int draw_cap, int stride, long long it, int* sample)
{
    int pos[MAX_SET], val[MAX_SET], n_mod = 0;
    unsigned int avail = (unsigned int)p.n;
    for (int k = 0; k < set; k++) {
        const unsigned int r32 = hs_ransac_draw(draws, draw_cap, stride, p.q, p.seed, it, set, k);
        const int randi = (int)(((unsigned long long)r32 * (unsigned long long)avail) >> 32);
        const int back = (int)avail - 1;
        int idx = randi, at_b = back, hit = -1;                    // hit: where the place randi is kept, if it is
        for (int m = 0; m < n_mod; m++) {
            if (pos[m] == randi) { idx = val[m]; hit = m; }
            if (pos[m] == back) at_b = val[m];
        }
        sample[k] = idx;
        const int place = WRITE_AT_VALUE ? idx : randi;            // the one difference
        if (!WRITE_AT_VALUE || (unsigned int)place < avail) {
            int slot = hit;
            if constexpr (WRITE_AT_VALUE) { slot = -1; for (int m = 0; m < n_mod; m++) if (pos[m] == place) slot = m; }
            if (slot < 0) { slot = n_mod++; pos[slot] = place; }
            val[slot] = at_b;
        }
        avail--;
    }
}

// mnIterations as a call reads it: a negative count (a state no call of this library and no hs_*_state_init wrote; the host form refuses it, the
// device form cannot see it) counts as 0, so no iteration index is negative and the draws table is never indexed below its start
HS_RANSAC_HD inline int hs_ransac_it0(int iterations) { return iterations < 0 ? 0 : iterations; }
// iterations a call of n_iterations runs from it0 when nothing returns early, never more than H, the bound the work area was carved for.  The two
// loop rules; with it0 = 0 and H = INT_MAX each is also the bound a problem planned to max_its contributes to the H of a call (hs_*_call_bound).
//   PnPsolver.cc:188    while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations)
HS_RANSAC_HD inline int hs_ransac_passes_or(int it0, int max_its, int n_iterations, int H)
{
    const int passes = it0 < max_its && max_its - it0 > n_iterations ? max_its - it0 : n_iterations;
    return passes < H ? passes : H;
}
//   Sim3Solver.cc:162   while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations)
HS_RANSAC_HD inline int hs_ransac_passes_and(int it0, int max_its, int n_iterations, int H)
{
    int passes = it0 < max_its ? max_its - it0 : 0;
    if (passes > n_iterations) passes = n_iterations;
    return passes < H ? passes : H;
}

// host side.  A launcher's loop: fn(q0, nb) for the problems q0 .. q0+nb-1 of one launch pair, `batch` at a time (their records travel as kernel arguments)
template <class Fn> inline void hs_ransac_for_batches(int Q, int batch, Fn fn)
{
    for (int q0 = 0; q0 < Q; q0 += batch) fn(q0, Q - q0 < batch ? Q - q0 : batch);
}

// the arguments of hs_*_iterate(_device) (include/hyslam_amd.h), host or device pointers by the form, but params and corr_offsets: always host
template <class Params, class Corr, class State, class Result> struct HsRansacArgs {
    using corr_t = Corr; using state_t = State; using result_t = Result;
    int Q; const Params* params; const int64_t* corr_offsets; const Corr* corrs; int n_iterations; const uint32_t* draws; int draw_cap;
    State* states; uint8_t* best_masks; Result* results; uint8_t* inlier_masks;
};

// A solver hands the bodies below a struct E of static members (HsPnpEntry, HsSim3Entry): draw_stride (words of a draws-table row), mask_inout (the
// host form uploads inlier_masks before it brings them back), state_init (the name of its hs_*_state_init, for one refusal), problem_why(params[q])
// (its own check of one problem: the refusal's text or nullptr), work_bytes(a) (the call's work area) and launch(a, d_work, stream) (its launcher).

// the predicate both forms share: pure host code over the by-value arguments and the two host arrays
template <class E, class A> inline const char* hs_ransac_iterate_why(const A& a, bool device)
{
    if (a.Q < 1 || !a.params || !a.corr_offsets || !a.states || !a.results) return "bad argument";
    if (a.n_iterations < 1) return "n_iterations must be positive";
    if (a.draw_cap < 0 || (a.draw_cap > 0 && !a.draws)) return "bad argument";
    if (!hs_csr_ok(a.corr_offsets, a.Q)) return "offsets must be non-negative and non-decreasing";
    if (a.corr_offsets[a.Q] > 0 && (!a.corrs || !a.best_masks || !a.inlier_masks)) return "bad argument";
    if (device && ((uintptr_t)a.corrs & 15)) return "d_corrs is 16-byte aligned";
    for (int q = 0; q < a.Q; q++) {
        if (const char* why = E::problem_why(a.params[q])) return why;
        if (a.corr_offsets[q + 1] - a.corr_offsets[q] > 0x7fffffff) return "a problem holds at most 2^31 - 1 correspondences";
    }
    return nullptr;
}

// hs_*_iterate_device: every pointer of `a` device memory but params and corr_offsets; enqueues on `stream` and returns
template <class E, class A> inline int hs_ransac_iterate_device(hs_orb* h, const A& a, void* d_work, void* stream)
{
    const char* why = hs_ransac_iterate_why<E>(a, true);
    if (!why && (!d_work || ((uintptr_t)d_work & 15))) why = "d_work is required and 16-byte aligned";
    return hs_device_call(h, why, stream, [&](hipStream_t s) { E::launch(a, d_work, s); });
}

// hs_*_iterate: host pointers, staged through HsStage, its work area included, so both forms run the same launches on the same layout
template <class E, class A> inline int hs_ransac_iterate_host(hs_orb* h, const A& a)
{
    if (!h) return HS_ERR_INVALID;
    if (const char* why = hs_ransac_iterate_why<E>(a, false)) return hs_fail(h, HS_ERR_INVALID, why);
    for (int q = 0; q < a.Q; q++)
        if (a.states[q].iterations < 0 || a.states[q].best_inliers < 0)
            return hs_fail(h, HS_ERR_INVALID, std::string("a state holds a negative count: start from ") + E::state_init);
    const size_t n_total = (size_t)a.corr_offsets[a.Q];
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    HsStage st(h);
    typename A::corr_t* d_corrs; uint32_t* d_draws; typename A::state_t* d_states; uint8_t *d_best, *d_inl, *d_work; typename A::result_t* d_res;
    st.in(&d_corrs, n_total, a.corrs);
    st.in(&d_draws, (size_t)a.Q * (size_t)a.draw_cap * E::draw_stride, a.draws);
    st.inout(&d_states, (size_t)a.Q, a.states);
    st.inout(&d_best, n_total, a.best_masks);
    st.out(&d_res, (size_t)a.Q, a.results);
    // PnP: the mask of a problem that returns no pose comes back as it went, so it goes up first.  Sim3: always written (Sim3Solver.cc:147).
    if (E::mask_inout) st.inout(&d_inl, n_total, a.inlier_masks);
    else st.out(&d_inl, n_total, a.inlier_masks);
    st.temp(&d_work, E::work_bytes(a));
    const int rc = st.begin();
    if (rc != HS_OK) return rc;
    E::launch(A{ a.Q, a.params, a.corr_offsets, d_corrs, a.n_iterations, a.draw_cap > 0 ? d_draws : nullptr, a.draw_cap, d_states, d_best, d_res, d_inl }, d_work,
              st.stream());
    return st.finish();
}
