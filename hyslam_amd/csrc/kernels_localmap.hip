// kernels_localmap.hip — the local map of TrackLocalMap (src/slam/tracking/TrackLocalMap.cpp) between the key-frame vote and the projection search:
// kernels and launchers of hs_local_keyframes, hs_local_points and hs_landmark_gather (entry points: hs_localmap.hip, include/hyslam_amd.h).
//
//   k_local_keyframes   the expansion of UpdateLocalKeyFrames (:106-156): ONE wave walks the live set in ascending slot order, as the reference
//                       iterates its std::set<KeyFrame*> while inserting into it
//   k_lp_mark           the head of SearchLocalPoints (:55-67): frame_remove, and a flag on every landmark the frame holds through a good association
//   k_lp_count          UpdateLocalPoints (:166-184) from the landmarks' side: keep flag per landmark, count per block
//   k_lp_scan           exclusive scan of the block counts, n_sel
//   k_lp_scatter        ascending landmark index -> sel; the tail of sel is -1
//   k_lm_query          the CSR offsets of the fused call's single vote query
//   k_landmark_gather   d_out[j] = d_lms[sel[j]] as five 16-byte pieces per record on consecutive lanes
//
// Integer and index work only: every result is identical to the reference's.  No position is decided by an atomic counter: the compaction is
// per-block counts, a scan and a scatter, so sel is the same on every run.
#include "hs_match_device.h"

#define LK_THREADS 64                        // one wave
#define LP_THREADS HS_LOCAL_POINTS_BLOCK     // block_scan_excl (hs_match_device.h) is written for 1024 threads
static_assert(LP_THREADS == 1024, "block_scan_excl is written for 1024 threads");
static_assert(sizeof(hs_landmark) == 80, "the gather moves an hs_landmark as five 16-byte pieces");

// the set lives in `local` (global memory) and is read back by the wave that wrote it: past the vector cache, like kf_count (hs_kfgraph.hip)
__device__ __forceinline__ int lk_member(const uint8_t* local, int i) { return __hip_atomic_load(local + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(LK_THREADS) void k_local_keyframes(int n_kf, const int32_t* weights, const uint8_t* kf_bad, const int32_t* neigh, int neigh_cap,
                                                                const int32_t* parent, int n_max, int n_neighbor, uint8_t* local, int32_t* n_local)
{
    const int lane = threadIdx.x;
    // local_key_frames = the counted key frames that are not bad (:109-123)
    int mine = 0;
    for (int i = lane; i < n_kf; i += LK_THREADS) {
        const int m = weights[i] > 0 && !kf_bad[i];
        local[i] = (uint8_t)m;
        mine += m;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) mine += __shfl_xor(mine, s, 64);
    long long size = mine;                                                             // uniform from here on
    __threadfence();
    // `local_key_frames.size() > params.N_max_local_keyframes` compares a size_t with an int: the int is converted (:130)
    const unsigned long long limit = (unsigned long long)(long long)n_max;
    n_neighbor = min(n_neighbor, neigh_cap);

    int cursor = -1;                                                                   // the walk: the smallest member above the cursor is next
    for (;;) {
        int next = -1;
        for (int base = (cursor + 1) & ~63; base < n_kf && next < 0; base += 64) {
            const int i = base + lane;
            const unsigned long long word = __ballot(i < n_kf && i > cursor && lk_member(local, i));
            if (word) next = base + __ffsll((long long)word) - 1;
        }
        if (next < 0) break;                                                           // itKF == itEndKF
        cursor = next;
        if ((unsigned long long)size > limit) break;                                   // (:130)
        // the first of the slot's n_neighbor best covisible key frames that is not bad (:137-147)
        int found = -1;
        for (int k0 = 0; k0 < n_neighbor && found < 0; k0 += 64) {
            const int k = k0 + lane;
            const int s = k < n_neighbor ? neigh[(size_t)cursor * neigh_cap + k] : -1;
            const unsigned long long ok = __ballot((unsigned)s < (unsigned)n_kf && !kf_bad[s]);
            if (ok) found = __shfl(s, __ffsll((long long)ok) - 1, 64);
        }
        const int par = parent[cursor];
        const int ins[2] = {found, (unsigned)par < (unsigned)n_kf ? par : -1};         // the parent goes in whether it is bad or not (:149-152)
#pragma unroll
        for (int t = 0; t < 2; t++) {
            if (ins[t] < 0 || lk_member(local, ins[t])) continue;
            if (lane == 0) __hip_atomic_store(local + ins[t], (uint8_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence();
            size++;
        }
        if (ins[1] >= 0) break;                                                        // the `break` at :153 leaves the outer loop
    }
    if (lane == 0) *n_local = (int32_t)size;
}

__global__ __launch_bounds__(256) void k_lp_mark(int L, const uint8_t* lm_bad, const int32_t* frame_lm, int n_assoc, uint8_t* frame_remove, uint8_t* flag)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= n_assoc) return;
    const int lm = frame_lm[a];
    if ((unsigned)lm >= (unsigned)L) { frame_remove[a] = 0; return; }                  // if(!pMP){continue;}
    const uint8_t bad = lm_bad[lm] ? 1 : 0;
    frame_remove[a] = bad;                                                             // removeLandMarkAssociation(LMid) (:62)
    if (!bad) flag[lm] = 1;                                                            // local_map_points.erase(pMP) (:65); every writer stores the same 1
}

// flag[lm]: in = held by the frame through a good association, out = selected.  One landmark per thread; the walk over its observations stops at the
// first local key frame.
__global__ __launch_bounds__(LP_THREADS) void k_lp_count(int L, int n_kf, const int64_t* lm_off, const int32_t* lm_kf, const uint8_t* lm_bad, const uint8_t* local,
                                                         uint8_t* flag, int32_t* block_cnt)
{
    __shared__ uint32_t s_wave[16];
    const int64_t lm = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
    uint32_t keep = 0;
    if (lm < L) {
        if (!lm_bad[lm] && !flag[lm]) {
            const int64_t oe = lm_off[lm + 1];
            for (int64_t j = lm_off[lm]; j < oe && !keep; j++) {
                const int s = lm_kf[j];
                keep = (unsigned)s < (unsigned)n_kf && local[s];
            }
        }
        flag[lm] = (uint8_t)keep;
    }
    uint32_t total;
    block_scan_excl(keep, s_wave, total);
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = (int32_t)total;
}

// block_cnt[b] -> the number of selected landmarks in the blocks before b; one workgroup
__global__ __launch_bounds__(LP_THREADS) void k_lp_scan(int n_blocks, int32_t* block_cnt, int32_t* n_sel)
{
    __shared__ uint32_t s_wave[16];
    uint32_t base = 0;
    for (int b0 = 0; b0 < n_blocks; b0 += LP_THREADS) {
        const int b = b0 + threadIdx.x;
        const uint32_t c = b < n_blocks ? (uint32_t)block_cnt[b] : 0u;
        uint32_t total;
        const uint32_t pos = block_scan_excl(c, s_wave, total);
        if (b < n_blocks) block_cnt[b] = (int32_t)(base + pos);
        base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_sel = (int32_t)base;
}

// blocks [0, n_blocks): the selected landmarks of the block at their positions; every block also fills its share of the tail of sel with -1
__global__ __launch_bounds__(LP_THREADS) void k_lp_scatter(int L, int n_blocks, const uint8_t* flag, const int32_t* block_off, const int32_t* n_sel, int32_t* sel, int cap)
{
    __shared__ uint32_t s_wave[16];
    if ((int)blockIdx.x < n_blocks) {
        const int64_t lm = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
        const uint32_t keep = lm < L ? flag[lm] : 0u;
        uint32_t total;
        const int64_t pos = (int64_t)block_off[blockIdx.x] + block_scan_excl(keep, s_wave, total);
        if (keep && pos < cap) sel[pos] = (int32_t)lm;
    }
    const int64_t stride = (int64_t)gridDim.x * LP_THREADS;
    for (int64_t j = (int64_t)*n_sel + (int64_t)blockIdx.x * LP_THREADS + threadIdx.x; j < cap; j += stride) sel[j] = -1;
}

// five consecutive lanes move one record; piece 2 holds normal[2], assoc_kp, prev_angle, skip
__global__ __launch_bounds__(256) void k_landmark_gather(const uint4* lms, int L, const int32_t* sel, const int32_t* n_sel, int cap, uint4* out)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t j = t / 5;
    const int piece = (int)(t - j * 5);
    if (j >= cap) return;
    const int src = j < *n_sel ? sel[j] : -1;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if ((unsigned)src < (unsigned)L) {
        v = lms[(int64_t)src * 5 + piece];
        if (piece == 2) { v.y = 0xFFFFFFFFu; v.w = 0u; }                                // assoc_kp = -1: no selected landmark is held by the frame; skip = 0
    } else if (piece == 2) { v.y = 0xFFFFFFFFu; v.w = 1u; }                             // past n_sel: an empty record with skip = 1
    out[j * 5 + piece] = v;
}

// the one query of the local-map vote: all of the frame's associations
__global__ void k_lm_query(int n_assoc, int64_t* q_off) { q_off[0] = 0; q_off[1] = n_assoc; }
void hs_launch_local_map_query(int n_assoc, int64_t* d_q_off, hipStream_t s) { hipLaunchKernelGGL(k_lm_query, dim3(1), dim3(1), 0, s, n_assoc, d_q_off); }

void hs_launch_local_keyframes(int n_kf, const int32_t* d_weights, const uint8_t* d_kf_bad, const int32_t* d_neigh, int neigh_cap, const int32_t* d_parent,
                               int n_max, int n_neighbor, uint8_t* d_local, int32_t* d_n_local, hipStream_t s)
{
    hipLaunchKernelGGL(k_local_keyframes, dim3(1), dim3(LK_THREADS), 0, s, n_kf, d_weights, d_kf_bad, d_neigh, neigh_cap, d_parent, n_max, n_neighbor, d_local, d_n_local);
}

void hs_launch_local_points(const hs_kf_table& T, const uint8_t* d_local, const int32_t* d_frame_lm, int n_assoc, uint8_t* d_frame_remove,
                            int32_t* d_sel, int cap, int32_t* d_n_sel, const HsLocalPointsWork& w, hipStream_t s)
{
    const int L = T.L, n_blocks = w.n_blocks;
    uint8_t* flag = w.flag;
    int32_t* block_cnt = w.block_cnt;
    if (L > 0) (void)hipMemsetAsync(flag, 0, (size_t)L, s);
    if (n_assoc > 0) hipLaunchKernelGGL(k_lp_mark, dim3((n_assoc + 255) / 256), dim3(256), 0, s, L, T.lm_bad, d_frame_lm, n_assoc, d_frame_remove, flag);
    if (n_blocks > 0) hipLaunchKernelGGL(k_lp_count, dim3(n_blocks), dim3(HS_LOCAL_POINTS_BLOCK), 0, s, L, T.n_kf, T.lm_obs_offsets, T.lm_obs_kf, T.lm_bad, d_local, flag, block_cnt);
    hipLaunchKernelGGL(k_lp_scan, dim3(1), dim3(HS_LOCAL_POINTS_BLOCK), 0, s, n_blocks, block_cnt, d_n_sel);
    hipLaunchKernelGGL(k_lp_scatter, dim3(std::max(n_blocks, 1)), dim3(HS_LOCAL_POINTS_BLOCK), 0, s, L, n_blocks, flag, block_cnt, d_n_sel, d_sel, cap);
}

void hs_launch_landmark_gather(const hs_landmark* d_lms, int L, const int32_t* d_sel, const int32_t* d_n_sel, int cap, hs_landmark* d_out, hipStream_t s)
{
    const int64_t threads = (int64_t)cap * 5;
    if (threads <= 0) return;
    hipLaunchKernelGGL(k_landmark_gather, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const uint4*>(d_lms), L, d_sel, d_n_sel, cap,
                       reinterpret_cast<uint4*>(d_out));
}
