// hs_kfgraph.hip — the key-frame graph walks over one observation table (landmark -> list of (key frame slot, octave)): kernels and entry points of
// hs_kf_votes(_device) and hs_kf_redundancy(_device) (include/hyslam_amd.h).
//
//   k_kf_votes       CovisNode::UpdateConnections (src/core/CovisibilityGraph.cpp:42-124) and TrackLocalMap::UpdateLocalKeyFrames
//                    (src/slam/tracking/TrackLocalMap.cpp:80-123): one workgroup per query — a histogram over the key-frame slots, the maximum, the
//                    entries that reach the threshold and their order
//   k_kf_redundancy  KeyFrameCuller::run (src/slam/mapping/KeyFrameCuller.cpp:33-86): one workgroup per candidate — a segmented count per item, an
//                    integer reduction, the verdict
//
// Integer arithmetic only (the verdict's one float product aside), so every path gives the reference's numbers whatever order the atomics arrive in.
// Where the reference's result depends on the walk order of a std::map<KeyFrame*, ...> the rule is spelled out on the slot: the maximum
// is reduced over the key (count, ~slot), the ordered list is ranked on the key (count, slot).
#include "hs_match_device.h"
#include "hs_track.h"               // hs_kf_votes_why / _enqueue: the vote is a stage of the local map and of the reference key frame
#include <climits>

#define KF_VOTE_THREADS 1024       // block_scan_excl (hs_match_device.h) is written for 1024 threads
#define KF_RED_THREADS 256

struct KfVoteArgs {
    int32_t L, n_kf, count_bad, th, cap, _r;
    const int64_t* lm_off; const int32_t* lm_kf; const uint8_t* lm_bad; const uint8_t* kf_bad; const int64_t* kf_id;
    const int64_t* q_off; const int32_t* q_lm; const int64_t* q_self;
    int32_t* weights;              // [Q][n_kf] or nullptr
    int32_t* counters;             // the global-counter instance: [Q][n_kf] (the weights rows when the caller wants them)
    int32_t *max_slot, *max_count, *ord_slot, *ord_w, *n_ord;
};

struct KfRedArgs {
    int32_t L, is_mono, th_obs; float frac;
    const int64_t* lm_off; const int32_t* lm_kf; const int32_t* lm_oct; const uint8_t* lm_bad; const int32_t* lm_nobs;
    const int32_t* cand_slot; const float* cand_th; const int64_t* cand_off;
    const int32_t* item_lm; const int32_t* item_oct; const float* item_depth;
    int32_t *n_mps, *n_red; uint8_t* cull;
};

// sum and 64-bit maximum over the workgroup; every thread gets both.  s_* hold one entry per wave and may be reused after the call.
template <int NW> __device__ __forceinline__ void kf_block_reduce(int& sum, unsigned long long& mx, int* s_sum, unsigned long long* s_mx)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) { sum += __shfl_xor(sum, s, 64); mx = max(mx, __shfl_xor(mx, s, 64)); }
    if ((tid & 63) == 0) { s_sum[tid >> 6] = sum; s_mx[tid >> 6] = mx; }
    __syncthreads();
    sum = 0; mx = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) { sum += s_sum[w]; mx = max(mx, s_mx[w]); }
    __syncthreads();
}

// a counter after the vote: LDS, or global memory that this workgroup's atomics have just written (read past the vector cache)
template <bool LDS> __device__ __forceinline__ int kf_count(const int32_t* cnt, int i)
{
    if (LDS) return cnt[i];
    return __hip_atomic_load(cnt + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS>
__global__ __launch_bounds__(KF_VOTE_THREADS) void k_kf_votes(const KfVoteArgs a)
{
    extern __shared__ int32_t s_cnt[];                           // LDS instance: n_kf counters
    __shared__ unsigned long long s_keys[HS_KF_SORT_PASS];
    __shared__ unsigned long long s_mx[16];
    __shared__ int s_sum[16];
    __shared__ uint32_t s_wave[16];
    const int q = blockIdx.x, tid = threadIdx.x, n_kf = a.n_kf;
    int32_t* cnt = LDS ? s_cnt : a.counters + (size_t)q * n_kf;

    for (int i = tid; i < n_kf; i += KF_VOTE_THREADS) cnt[i] = 0;
    if (!LDS) __threadfence();
    __syncthreads();

    // KFcounter[pKF_obs]++ / keyframeCounter[pKF]++: one landmark of the query per thread
    const int64_t self = a.q_self ? a.q_self[q] : -1;
    const int64_t qe = a.q_off[q + 1];
    for (int64_t k = a.q_off[q] + tid; k < qe; k += KF_VOTE_THREADS) {
        const int lm = a.q_lm[k];
        if ((unsigned)lm >= (unsigned)a.L || a.lm_bad[lm]) continue;                   // pMP->isBad() (:55)
        const int64_t oe = a.lm_off[lm + 1];
        for (int64_t j = a.lm_off[lm]; j < oe; j++) {
            const int s = a.lm_kf[j];
            if ((unsigned)s >= (unsigned)n_kf) continue;
            if (self != -1 && a.kf_id[s] == self) continue;                            // pKF_obs->mnId == pKF_node->mnId (:63)
            if (!a.count_bad && a.kf_bad[s]) continue;                                 // pKF_obs->isBad() (:65)
            atomicAdd(&cnt[s], 1);
        }
    }
    if (!LDS) __threadfence();
    __syncthreads();

    // `if (count > nmax)` on ascending slots = the largest (count, ~slot); a bad key frame is not a candidate (TrackLocalMap.cpp:113)
    const int th = a.th;
    unsigned long long best = 0;
    int listed = 0;
    for (int i = tid; i < n_kf; i += KF_VOTE_THREADS) {
        const int c = kf_count<LDS>(cnt, i);
        if (c <= 0 || (a.count_bad && a.kf_bad[i])) continue;
        best = max(best, ((unsigned long long)(unsigned)c << 32) | (0xFFFFFFFFu - (unsigned)i));
        listed += c >= th;
    }
    kf_block_reduce<16>(listed, best, s_sum, s_mx);
    const int max_count = (int)(best >> 32), max_slot = best ? (int)(0xFFFFFFFFu - (unsigned)best) : -1;
    const int n_ord = listed ? listed : (best ? 1 : 0);
    const int cap = a.cap;
    int32_t* os = a.ord_slot + (size_t)q * cap;
    int32_t* ow = a.ord_w + (size_t)q * cap;

    if (cap > 0 && listed == 0) {                                                      // vPairs.empty(): (nmax, pKFmax) alone (:100-104)
        if (tid == 0 && best) { os[0] = max_slot; ow[0] = max_count; }
    } else if (cap > 0 && listed <= HS_KF_SORT_PASS) {
        // the entries in ascending slot order, as the walk over KFcounter pushes them (:86-98) ...
        uint32_t base = 0;
        for (int i0 = 0; i0 < n_kf; i0 += KF_VOTE_THREADS) {
            const int i = i0 + tid;
            const int c = i < n_kf ? kf_count<LDS>(cnt, i) : 0;
            const bool on = c > 0 && c >= th && !(a.count_bad && a.kf_bad[i]);
            uint32_t total;
            const uint32_t pos = block_scan_excl(on ? 1u : 0u, s_wave, total);
            if (on) s_keys[base + pos] = ((unsigned long long)(unsigned)c << 32) | (unsigned)i;
            base += total;
            __syncthreads();
        }
        // ... and sort + push_front (:106-113): position = number of entries with a larger (weight, slot)
        for (int i = tid; i < listed; i += KF_VOTE_THREADS) {
            const unsigned long long key = s_keys[i];
            int rank = 0;
            for (int j = 0; j < listed; j++) rank += s_keys[j] > key;
            if (rank < cap) { os[rank] = (int)(unsigned)key; ow[rank] = (int)(key >> 32); }
        }
    } else if (cap > 0) {
        // longer than one pass holds: the same rank, counted over the counters themselves
        for (int i = tid; i < n_kf; i += KF_VOTE_THREADS) {
            const int c = kf_count<LDS>(cnt, i);
            if (c <= 0 || c < th || (a.count_bad && a.kf_bad[i])) continue;
            const unsigned long long key = ((unsigned long long)(unsigned)c << 32) | (unsigned)i;
            int rank = 0;
            for (int j = 0; j < n_kf; j++) {
                const int cj = kf_count<LDS>(cnt, j);
                if (cj <= 0 || cj < th || (a.count_bad && a.kf_bad[j])) continue;
                rank += (((unsigned long long)(unsigned)cj << 32) | (unsigned)j) > key;
            }
            if (rank < cap) { os[rank] = i; ow[rank] = c; }
        }
    }
    for (int i = min(n_ord, cap) + tid; i < cap; i += KF_VOTE_THREADS) { os[i] = -1; ow[i] = 0; }
    if (LDS && a.weights) {
        int32_t* w = a.weights + (size_t)q * n_kf;
        for (int i = tid; i < n_kf; i += KF_VOTE_THREADS) w[i] = cnt[i];
    }
    if (tid == 0) { a.max_slot[q] = max_slot; a.max_count[q] = max_count; a.n_ord[q] = n_ord; }
}

__global__ __launch_bounds__(KF_RED_THREADS) void k_kf_redundancy(const KfRedArgs a)
{
    __shared__ int s_mps[KF_RED_THREADS / 64], s_red[KF_RED_THREADS / 64];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int me = a.cand_slot[c];
    const float th_depth = a.cand_th[c];
    const int th_obs = a.th_obs;
    int n_mps = 0, n_red = 0;
    const int64_t ke = a.cand_off[c + 1];
    for (int64_t k = a.cand_off[c] + tid; k < ke; k += KF_RED_THREADS) {
        const int lm = a.item_lm[k];
        if ((unsigned)lm >= (unsigned)a.L || a.lm_bad[lm]) continue;                   // pMP && !pMP->isBad() (:42-44)
        if (!a.is_mono) {
            const float d = a.item_depth[k];
            if (d > th_depth || d < 0.0f) continue;                                    // (:50)
        }
        n_mps++;
        if (a.lm_nobs[lm] <= th_obs) continue;                                         // pMP->Observations() > thObs (:55)
        const int level = a.item_oct[k];
        int n = 0;
        const int64_t oe = a.lm_off[lm + 1];
        for (int64_t j = a.lm_off[lm]; j < oe; j++)
            n += a.lm_kf[j] != me && a.lm_oct[j] <= level + 1;                         // (:63,69); the `break` at thObs changes no verdict
        n_red += n >= th_obs;
    }
    // both counts in one integer sum over the workgroup: lanes, then the waves' partial sums through LDS
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) { n_mps += __shfl_xor(n_mps, s, 64); n_red += __shfl_xor(n_red, s, 64); }
    if ((tid & 63) == 0) { s_mps[tid >> 6] = n_mps; s_red[tid >> 6] = n_red; }
    __syncthreads();
    if (tid == 0) {
        n_mps = 0; n_red = 0;
#pragma unroll
        for (int w = 0; w < KF_RED_THREADS / 64; w++) { n_mps += s_mps[w]; n_red += s_red[w]; }
        a.n_mps[c] = n_mps; a.n_red[c] = n_red;
        a.cull[c] = (float)n_red > __fmul_rn(a.frac, (float)n_mps) ? 1 : 0;            // nRedundantObservations > params.frac_redundant * nMPs (:86)
    }
}

static void launch_votes(const KfVoteArgs& a, int Q, hipStream_t s)
{
    if (a.n_kf <= HS_KF_LDS_SLOTS) hipLaunchKernelGGL(k_kf_votes<true>, dim3(Q), dim3(KF_VOTE_THREADS), (size_t)std::max(a.n_kf, 1) * sizeof(int32_t), s, a);
    else hipLaunchKernelGGL(k_kf_votes<false>, dim3(Q), dim3(KF_VOTE_THREADS), 0, s, a);
}

void hs_kf_votes_enqueue(const hs_kf_table* T, int Q, const int64_t* d_q_offsets, const int32_t* d_q_lm, const int64_t* d_q_self_id, int count_bad_kf, int th,
                         int32_t* d_weights, int32_t* d_max_slot, int32_t* d_max_count, int32_t* d_ordered_slot, int32_t* d_ordered_weight, int cap, int32_t* d_n_ordered,
                         hipStream_t s)
{
    if (Q == 0) return;
    const KfVoteArgs a{T->L, T->n_kf, count_bad_kf ? 1 : 0, th, cap, 0, T->lm_obs_offsets, T->lm_obs_kf, T->lm_bad, T->kf_bad, T->kf_id,
                       d_q_offsets, d_q_lm, d_q_self_id, d_weights, d_weights, d_max_slot, d_max_count, d_ordered_slot, d_ordered_weight, d_n_ordered};
    launch_votes(a, Q, s);
}

extern "C" {

int hs_kf_votes_device(hs_orb* h, const hs_kf_table* T, int Q, const int64_t* d_q_offsets, const int32_t* d_q_lm, const int64_t* d_q_self_id,
                       int count_bad_kf, int th, int32_t* d_weights, int32_t* d_max_slot, int32_t* d_max_count,
                       int32_t* d_ordered_slot, int32_t* d_ordered_weight, int cap, int32_t* d_n_ordered, void* stream)
{
    return hs_device_call(h, hs_kf_votes_why(T, Q, d_q_offsets, d_weights, d_max_slot, d_max_count, d_ordered_slot, d_ordered_weight, cap, d_n_ordered), stream,
                          [&](hipStream_t s) {
        hs_kf_votes_enqueue(T, Q, d_q_offsets, d_q_lm, d_q_self_id, count_bad_kf, th, d_weights, d_max_slot, d_max_count, d_ordered_slot, d_ordered_weight, cap,
                            d_n_ordered, s);
    });
}

int hs_kf_votes(hs_orb* h, const hs_kf_table* T, int Q, const int64_t* q_offsets, const int32_t* q_lm, const int64_t* q_self_id,
                int count_bad_kf, int th, int32_t* weights, int32_t* max_slot, int32_t* max_count,
                int32_t* ordered_slot, int32_t* ordered_weight, int cap, int32_t* n_ordered)
{
    if (!h) return HS_ERR_INVALID;
    if (!T || Q < 0 || cap < 0 || T->L < 0 || T->n_kf < 0) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (Q == 0) return HS_OK;
    const int L = T->L, n_kf = T->n_kf;
    if (!T->lm_obs_offsets || !q_offsets || !max_slot || !max_count || !n_ordered || (cap > 0 && (!ordered_slot || !ordered_weight)) ||
        (n_kf > 0 && (!T->kf_bad || !T->kf_id)) || (L > 0 && !T->lm_bad))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (!hs_csr_ok(T->lm_obs_offsets, L) || !hs_csr_ok(q_offsets, Q)) return hs_fail(h, HS_ERR_INVALID, "offsets must be non-negative and non-decreasing");
    const size_t n_obs = (size_t)T->lm_obs_offsets[L], n_q = (size_t)q_offsets[Q];
    if ((n_obs > 0 && !T->lm_obs_kf) || (n_q > 0 && !q_lm)) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (!hs_index_range_ok(T->lm_obs_kf, n_obs, 0, n_kf) || !hs_index_range_ok(q_lm, n_q, 0, L)) return hs_fail(h, HS_ERR_INVALID, "a key-frame slot or landmark index outside the table");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    HsStage st(h);
    KfVoteArgs a{L, n_kf, count_bad_kf ? 1 : 0, th, cap, 0};
    int64_t *d_lm_off, *d_kf_id, *d_q_off, *d_self;
    int32_t *d_lm_kf, *d_q_lm;
    uint8_t *d_lm_bad, *d_kf_bad;
    st.in(&d_lm_off, (size_t)L + 1, T->lm_obs_offsets); st.in(&d_lm_kf, n_obs, T->lm_obs_kf); st.in(&d_lm_bad, (size_t)L, T->lm_bad);
    st.in(&d_kf_bad, (size_t)n_kf, T->kf_bad); st.in(&d_kf_id, (size_t)n_kf, T->kf_id);
    st.in(&d_q_off, (size_t)Q + 1, q_offsets); st.in(&d_q_lm, n_q, q_lm); st.in(&d_self, (size_t)Q, q_self_id);
    const size_t n_w = (size_t)Q * n_kf;
    if (weights) st.out(&a.weights, n_w, weights);
    else st.temp(&a.weights, n_kf > HS_KF_LDS_SLOTS ? n_w : 0);                       // the global-counter rows nobody asked to see
    st.out(&a.max_slot, (size_t)Q, max_slot); st.out(&a.max_count, (size_t)Q, max_count);
    st.out(&a.ord_slot, (size_t)Q * cap, ordered_slot); st.out(&a.ord_w, (size_t)Q * cap, ordered_weight); st.out(&a.n_ord, (size_t)Q, n_ordered);
    const int rc = st.begin();
    if (rc != HS_OK) return rc;
    a.lm_off = d_lm_off; a.lm_kf = d_lm_kf; a.lm_bad = d_lm_bad; a.kf_bad = d_kf_bad; a.kf_id = d_kf_id;
    a.q_off = d_q_off; a.q_lm = d_q_lm; a.q_self = q_self_id ? d_self : nullptr;
    a.counters = a.weights;
    if (!weights) a.weights = nullptr;
    launch_votes(a, Q, st.stream());
    return st.finish();
}

int hs_kf_redundancy_device(hs_orb* h, const hs_kf_table* T, int C, const int32_t* d_cand_slot, const float* d_cand_th_depth,
                            const int64_t* d_cand_offsets, const int32_t* d_item_lm, const int32_t* d_item_octave, const float* d_item_depth,
                            int is_mono, int th_obs, float frac_redundant, int32_t* d_n_mps, int32_t* d_n_redundant, uint8_t* d_cull, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!T || C < 0 || T->L < 0) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (C == 0) return HS_OK;
    if (!T->lm_obs_offsets || !d_cand_slot || !d_cand_th_depth || !d_cand_offsets || !d_n_mps || !d_n_redundant || !d_cull ||
        (T->L > 0 && (!T->lm_bad || !T->lm_nobs)))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    const KfRedArgs a{T->L, is_mono ? 1 : 0, th_obs, frac_redundant, T->lm_obs_offsets, T->lm_obs_kf, T->lm_obs_octave, T->lm_bad, T->lm_nobs,
                      d_cand_slot, d_cand_th_depth, d_cand_offsets, d_item_lm, d_item_octave, d_item_depth, d_n_mps, d_n_redundant, d_cull};
    hipLaunchKernelGGL(k_kf_redundancy, dim3(C), dim3(KF_RED_THREADS), 0, hs_stream_or(h, stream), a);
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_kf_redundancy(hs_orb* h, const hs_kf_table* T, int C, const int32_t* cand_slot, const float* cand_th_depth, const int64_t* cand_offsets,
                     const int32_t* item_lm, const int32_t* item_octave, const float* item_depth, int is_mono, int th_obs, float frac_redundant,
                     int32_t* n_mps, int32_t* n_redundant, uint8_t* cull)
{
    if (!h) return HS_ERR_INVALID;
    if (!T || C < 0 || T->L < 0) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (C == 0) return HS_OK;
    const int L = T->L;
    if (!T->lm_obs_offsets || !cand_slot || !cand_th_depth || !cand_offsets || !n_mps || !n_redundant || !cull || (L > 0 && (!T->lm_bad || !T->lm_nobs)))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (!hs_csr_ok(T->lm_obs_offsets, L) || !hs_csr_ok(cand_offsets, C)) return hs_fail(h, HS_ERR_INVALID, "offsets must be non-negative and non-decreasing");
    const size_t n_obs = (size_t)T->lm_obs_offsets[L], n_it = (size_t)cand_offsets[C];
    if ((n_obs > 0 && (!T->lm_obs_kf || !T->lm_obs_octave)) || (n_it > 0 && (!item_lm || !item_octave || (!is_mono && !item_depth))))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (!hs_index_range_ok(item_lm, n_it, 0, L)) return hs_fail(h, HS_ERR_INVALID, "a landmark index outside the table");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    HsStage st(h);
    KfRedArgs a{L, is_mono ? 1 : 0, th_obs, frac_redundant};
    int64_t *d_lm_off, *d_c_off;
    int32_t *d_lm_kf, *d_lm_oct, *d_nobs, *d_slot, *d_ilm, *d_ioct;
    uint8_t* d_lm_bad;
    float *d_th, *d_depth;
    st.in(&d_lm_off, (size_t)L + 1, T->lm_obs_offsets); st.in(&d_lm_kf, n_obs, T->lm_obs_kf); st.in(&d_lm_oct, n_obs, T->lm_obs_octave);
    st.in(&d_lm_bad, (size_t)L, T->lm_bad); st.in(&d_nobs, (size_t)L, T->lm_nobs);
    st.in(&d_slot, (size_t)C, cand_slot); st.in(&d_th, (size_t)C, cand_th_depth); st.in(&d_c_off, (size_t)C + 1, cand_offsets);
    st.in(&d_ilm, n_it, item_lm); st.in(&d_ioct, n_it, item_octave); st.in(&d_depth, is_mono ? 0 : n_it, item_depth);
    st.out(&a.n_mps, (size_t)C, n_mps); st.out(&a.n_red, (size_t)C, n_redundant); st.out(&a.cull, (size_t)C, cull);
    const int rc = st.begin();
    if (rc != HS_OK) return rc;
    a.lm_off = d_lm_off; a.lm_kf = d_lm_kf; a.lm_oct = d_lm_oct; a.lm_bad = d_lm_bad; a.lm_nobs = d_nobs;
    a.cand_slot = d_slot; a.cand_th = d_th; a.cand_off = d_c_off; a.item_lm = d_ilm; a.item_oct = d_ioct; a.item_depth = d_depth;
    hipLaunchKernelGGL(k_kf_redundancy, dim3(C), dim3(KF_RED_THREADS), 0, st.stream(), a);
    return st.finish();
}

}  // extern "C"
