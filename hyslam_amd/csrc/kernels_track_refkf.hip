// kernels_track_refkf.hip — the two steps of TrackReferenceKeyFrame::track that had no resident form (entry points in hs_track_refkf.hip,
// include/hyslam_amd.h):
//
//   k_refkf_match          the node walk and BestMatchBoWCriterion of SearchByBoW(KeyFrame*, Frame&)   src/features/FeatureMatcher.cc:216-265
//   k_refkf_finish         RotationConsistencyBoW, matches_internal.size(), matches[idx_f] = lm         FeatureMatcher.cc:266-277, MatchCriteria.cpp:679-726
//   k_vassoc_*             Frame::associateLandMarks(matches, true) as a closed form                    src/core/Frame.cc:221-232, LandMarkMatches.cpp:26-51
//
// The search.  A keypoint belongs to the feature-vector node its `node` entry names; a keypoint whose word weight is not positive (where a weight
// array is given) or whose node is negative belongs to none (DBoW2: `if (w > 0) fv.addFeature(nid, i)`).  The reference visits the nodes both
// feature vectors hold and, inside one, every key-frame index against the frame's indices of the same node in ascending order, first minimum
// wins.  A key-frame keypoint sits in one node, so its answer does not depend on the walk: one wavefront per key-frame keypoint scans the frame's
// node array, and the candidate key dist << 32 | frame index makes the smallest key the reference's first minimum.  No list crosses the interface.
//
// The replay in view order.  Ops run in ascending view index, a view has at most one op and a landmark at most one.  With kp0 = the state before:
//   * only the op of landmark m erases a holder of m, and a view is overwritten by its own op alone, so at the time of op (i, m) the holders of m
//     are H(m) = { v : kp0[v] == m and (v has no op or v >= i) }; hasAssociation(m) = idx_old(m) = min H(m)
//   * view i is empty when its op runs  <=>  kp0[i] < 0, or the op of kp0[i] sits on a view i' < i and idx_old(kp0[i]) == i (it was erased)
//   * op (i, m) is the fresh insert (n_matches grows, a stale outliers entry stays)  <=>  view i is empty then and H(m) is empty
//   * an op view ends at its landmark (no later op erases it: that op's landmark differs); a view without an op ends at -1  <=>  it is idx_old of
//     its landmark's op
// Four phases with a kernel boundary between them; integer atomicMin only, plain stores where the preconditions make the writer unique.
#include "hs_track.h"
#include "hs_match_device.h"

namespace {
constexpr int VA_NONE = 0x7FFFFFFF;

// the key frame's keypoint range, read on the device: a slot outside [0, n_kf) or an empty key frame gives nk = 0
__device__ __forceinline__ void refkf_range(const hs_kf_features& K, const int32_t* __restrict__ kf_slot, int kf_cap, int64_t& off, int& nk)
{
    const int s = *kf_slot;
    off = 0; nk = 0;
    if ((unsigned)s >= (unsigned)K.n_kf) return;
    const int64_t a = K.kf_off[s], b = K.kf_off[s + 1];
    if (a < 0 || b <= a) return;
    off = a;
    nk = (int)min((int64_t)kf_cap, b - a);                      // a longer key frame is truncated in ascending index
}

// one wavefront per key-frame keypoint j < kf_cap; match_kf[j] = the frame view it takes, or -1 (every entry is written)
__global__ __launch_bounds__(256) void k_refkf_match(hs_kf_features K, const int32_t* __restrict__ kf_slot, int kf_cap, int L, const uint8_t* __restrict__ lm_bad,
                                                     const uint8_t* __restrict__ desc, const int32_t* __restrict__ node, const float* __restrict__ weight, int n,
                                                     float th_low, float nnratio, int32_t* __restrict__ match_kf)
{
    const int lane = threadIdx.x & 63;
    const int j = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (j >= kf_cap) return;
    int64_t off; int nk;
    refkf_range(K, kf_slot, kf_cap, off, nk);
    int found = -1;
    if (j < nk) {
        const int lm = K.kp_lm[off + j], nd = K.node[off + j];
        const bool in_fv = nd >= 0 && (!K.weight || K.weight[off + j] > 0.0f);            // `if (w > 0) fv.addFeature(nid, i)`
        if (in_fv && (unsigned)lm < (unsigned)L && !lm_bad[lm]) {                         // PreviouslyMatchedIndexCriterion(true)
            const Desc256 a = desc_load(K.desc + (size_t)(off + j) * 32);
            unsigned long long best = HS_NO_KEY; int second = HS_NO_DIST;
            for (int f = lane; f < n; f += 64) {
                if (node[f] != nd || (weight && !(weight[f] > 0.0f))) continue;
                const int d = hamming256(a, desc_load(desc + (size_t)f * 32));
                best2_take(best, second, ((unsigned long long)d << 32) | (unsigned)f, d);
            }
            wave_best2(best, second);
            if (best != HS_NO_KEY && bow_accept(best, second, th_low, nnratio)) found = (int)(best & 0xFFFFFFFFu);
        }
    }
    if (lane == 0) match_kf[j] = found;
}

// one workgroup: the rotation histogram over the matches, the count, and the collapse onto the frame's views (the largest idx_kf of a view wins:
// the std::map walk is ascending and `matches[idx_f] = lm` overwrites).  op_view doubles as the winner table between the two barriers.
__global__ __launch_bounds__(1024) void k_refkf_finish(hs_kf_features K, const int32_t* __restrict__ kf_slot, int kf_cap, const hs_keypoint* __restrict__ kps, int n,
                                                       int32_t* __restrict__ match_kf, int32_t* __restrict__ op_view, int32_t* __restrict__ op_lm,
                                                       int32_t* __restrict__ n_matches)
{
    __shared__ int hist[30];
    __shared__ int ind[3];
    __shared__ int total;
    const int tid = threadIdx.x;
    int64_t off; int nk;
    refkf_range(K, kf_slot, kf_cap, off, nk);
    if (tid < 30) hist[tid] = 0;
    if (tid == 0) total = 0;
    for (int f = tid; f < n; f += 1024) __hip_atomic_store(&op_view[f], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the atomicMax below meets it in L2
    __syncthreads();
    auto bin_of = [&](int j) { return rot_bin(kps[match_kf[j]].angle, K.kps[off + j].angle); };      // rot = frame angle - key-frame angle
    for (int j = tid; j < nk; j += 1024) if (match_kf[j] >= 0) { const int b = bin_of(j); if (b >= 0 && b < 30) atomicAdd(&hist[b], 1); }
    __syncthreads();
    if (tid == 0) three_maxima(hist, ind);
    __syncthreads();
    int kept = 0;
    for (int j = tid; j < nk; j += 1024) {
        const int f = match_kf[j];
        if (f < 0) continue;
        const int b = bin_of(j);
        if (b >= 0 && b < 30 && (b == ind[0] || b == ind[1] || b == ind[2])) { kept++; atomicMax(&op_view[f], j); }      // ind[k] == -1 names no bin (the reference asserts the range)
        else match_kf[j] = -1;
    }
    if (kept) atomicAdd(&total, kept);
    __syncthreads();
    for (int f = tid; f < n; f += 1024) {
        const int w = __hip_atomic_load(&op_view[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the atomics above ran in L2
        op_lm[f] = w >= 0 ? K.kp_lm[off + w] : -1;
        op_view[f] = w >= 0 ? f : -1;
    }
    if (tid == 0) *n_matches = total;
}

// ---- the replay in view order.  work: view_op [n] (the landmark of the view's op, -1 = none), lm_view [L] (the view of the landmark's op),
// idx_old [L]; the two [L] arrays are initialised only where the call can read them
__device__ __forceinline__ bool va_valid(int v, int k, int n, int L) { return (unsigned)v < (unsigned)n && (unsigned)k < (unsigned)L; }
__global__ __launch_bounds__(HS_TRACK_BLOCK) void k_vassoc_init(int n, int L, const int32_t* __restrict__ kp_lm, const int32_t* __restrict__ op_lm,
                                                                int32_t* __restrict__ view_op, int32_t* __restrict__ lm_view, int32_t* __restrict__ idx_old)
{
    const int t = blockIdx.x * HS_TRACK_BLOCK + threadIdx.x;
    if (t >= n) return;
    view_op[t] = -1;
    const int k = kp_lm[t], m = op_lm[t];
    if ((unsigned)k < (unsigned)L) { lm_view[k] = VA_NONE; idx_old[k] = VA_NONE; }
    if ((unsigned)m < (unsigned)L) { lm_view[m] = VA_NONE; idx_old[m] = VA_NONE; }
}
__global__ __launch_bounds__(HS_TRACK_BLOCK) void k_vassoc_ops(int n, int L, const int32_t* __restrict__ op_view, const int32_t* __restrict__ op_lm,
                                                               int32_t* __restrict__ view_op, int32_t* __restrict__ lm_view)
{
    const int j = blockIdx.x * HS_TRACK_BLOCK + threadIdx.x;
    if (j >= n) return;
    const int v = op_view[j], m = op_lm[j];
    if (!va_valid(v, m, n, L)) return;
    view_op[v] = m; lm_view[m] = v;                              // unique writers: a view in at most one op, a landmark in at most one
}
__global__ __launch_bounds__(HS_TRACK_BLOCK) void k_vassoc_holders(int n, int L, const int32_t* __restrict__ kp_lm, const int32_t* __restrict__ view_op,
                                                                   const int32_t* __restrict__ lm_view, int32_t* __restrict__ idx_old)
{
    const int v = blockIdx.x * HS_TRACK_BLOCK + threadIdx.x;
    if (v >= n) return;
    const int k = kp_lm[v];
    if ((unsigned)k >= (unsigned)L) return;
    const int i = lm_view[k];
    if (i != VA_NONE && (view_op[v] < 0 || v >= i)) atomicMin(&idx_old[k], v);
}
__global__ __launch_bounds__(HS_TRACK_BLOCK) void k_vassoc_final(int n, int L, int32_t* __restrict__ kp_lm, uint8_t* __restrict__ kp_outl, int32_t* __restrict__ n_matches,
                                                                 const int32_t* __restrict__ view_op, const int32_t* __restrict__ lm_view,
                                                                 const int32_t* __restrict__ idx_old)
{
    const int v = blockIdx.x * HS_TRACK_BLOCK + threadIdx.x;
    bool fresh = false;
    if (v < n) {
        const int m = view_op[v], k = kp_lm[v];
        const bool held = (unsigned)k < (unsigned)L;
        const bool erased = held && lm_view[k] != VA_NONE && idx_old[k] == v;        // views_to_landmarks.erase(idx_old): outliers and n_matches stay
        if (m >= 0) {
            fresh = (k < 0 || (erased && lm_view[k] < v)) && idx_old[m] == VA_NONE;
            kp_lm[v] = m;
            if (!(fresh && kp_outl[v])) kp_outl[v] = 1;                              // insert({i, false}) keeps a stale entry; the replace branch sets false
        } else if (erased) kp_lm[v] = -1;
    }
    const int c = __popcll(__ballot(fresh));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(n_matches, c);
}

}  // namespace

static dim3 rk_grid(int n) { return dim3((unsigned)((std::max(n, 1) + HS_TRACK_BLOCK - 1) / HS_TRACK_BLOCK)); }

void hs_launch_search_by_bow_kf(const hs_kf_features& K, const int32_t* d_kf_slot, const hs_kf_table& T, const hs_keypoint* d_kps, const uint8_t* d_desc,
                                const int32_t* d_node, const float* d_weight, int n, float th_low, float nnratio, int32_t* d_match_kf, int kf_cap, int32_t* d_op_view,
                                int32_t* d_op_lm, int32_t* d_n_matches, hipStream_t s)
{
    if (kf_cap > 0)
        hipLaunchKernelGGL(k_refkf_match, dim3((unsigned)((kf_cap + 3) / 4)), dim3(256), 0, s, K, d_kf_slot, kf_cap, T.L, T.lm_bad, d_desc, d_node, d_weight, n, th_low,
                           nnratio, d_match_kf);
    hipLaunchKernelGGL(k_refkf_finish, dim3(1), dim3(1024), 0, s, K, d_kf_slot, kf_cap, d_kps, n, d_match_kf, d_op_view, d_op_lm, d_n_matches);
}

void hs_launch_frame_associate_views(int n, int L, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, const int32_t* d_op_view, const int32_t* d_op_lm,
                                     const HsVassocWork& w, hipStream_t s)
{
    if (n <= 0) return;
    int32_t *view_op = w.view_op, *lm_view = w.lm_view, *idx_old = w.idx_old;
    hipLaunchKernelGGL(k_vassoc_init, rk_grid(n), dim3(HS_TRACK_BLOCK), 0, s, n, L, d_kp_lm, d_op_lm, view_op, lm_view, idx_old);
    hipLaunchKernelGGL(k_vassoc_ops, rk_grid(n), dim3(HS_TRACK_BLOCK), 0, s, n, L, d_op_view, d_op_lm, view_op, lm_view);
    hipLaunchKernelGGL(k_vassoc_holders, rk_grid(n), dim3(HS_TRACK_BLOCK), 0, s, n, L, d_kp_lm, view_op, lm_view, idx_old);
    hipLaunchKernelGGL(k_vassoc_final, rk_grid(n), dim3(HS_TRACK_BLOCK), 0, s, n, L, d_kp_lm, d_kp_outl, d_n_matches, view_op, lm_view, idx_old);
}
