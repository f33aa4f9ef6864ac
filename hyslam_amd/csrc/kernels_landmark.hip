// kernels_landmark.hip — a landmark's representative descriptor for a whole batch of landmarks.
//
//   k_landmark_small   MapPointDBEntry::_computeDistinctiveDescriptor_, N <= 64       src/core/MapPointDB.cpp:128-175
//   k_landmark_large   the same, N > 64
//
// Input is CSR: landmark i owns descriptors desc[off[i] .. off[i+1]) in the caller's order (the reference walks a std::map<KeyFrame*, ...>).
// Row r of the N x N Hamming matrix (diagonal 0 included) has the median element (size_t)(0.5*(N-1)) = (N-1)/2 of its ascending order; the
// reference keeps the first row whose median is strictly smaller than every earlier one.  Distances are integers in [0, 256], so the k-th
// smallest of a row is found by counting, not by sorting:
//   small: one wavefront per landmark, lane j holds descriptor j; per row a 9-step bisection over the value, count(d <= v) by one ballot.
//   large: one workgroup per landmark, one wavefront per row; the row is counted into a 257-bin LDS histogram and the k-th bin read off a
//          wave prefix sum.  LDS does not grow with N, so N is bounded only by memory (and by best[]'s int32).
// Both keep the reference's first-strict-minimum by minimising the key median << 32 | row.
#include "hs_internal.h"
#include <algorithm>

#define LM_SMALL 64            // largest N of the wave path
#define LM_LARGE_WAVES 8       // wavefronts per workgroup of the large path
#define LM_HIST 260            // 257 bins (distance 0..256) rounded up to a multiple of 4: each wave's histogram stays 16-byte aligned

// the wave's earlier LDS accesses are done before its next ones (all lanes): compiler barrier + lgkmcnt(0)
#define LM_WAVE_LDS_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                                __builtin_amdgcn_s_waitcnt(0xc07f); } while (0)

struct LmDesc { unsigned long long w[4]; };

__device__ __forceinline__ LmDesc lm_load(const uint8_t* __restrict__ desc, long long j)
{
    const ulonglong2* p = reinterpret_cast<const ulonglong2*>(desc + j * 32);
    const ulonglong2 a = p[0], b = p[1];
    return LmDesc{{a.x, a.y, b.x, b.y}};
}

__device__ __forceinline__ int lm_dist(const LmDesc& a, const LmDesc& b)
{
    return __popcll(a.w[0] ^ b.w[0]) + __popcll(a.w[1] ^ b.w[1]) + __popcll(a.w[2] ^ b.w[2]) + __popcll(a.w[3] ^ b.w[3]);
}

__device__ __forceinline__ void lm_write(int i, int n, int best, int median, int32_t* __restrict__ best_idx, int32_t* __restrict__ best_median)
{
    best_idx[i] = n > 0 ? best : -1;
    best_median[i] = n > 0 ? median : -1;
}

// N <= 64 (and the empty landmarks): four landmarks per 256-thread block, one per wavefront
__global__ __launch_bounds__(256) void k_landmark_small(const int64_t* __restrict__ off, const uint8_t* __restrict__ desc, int L,
                                                        int32_t* __restrict__ best_idx, int32_t* __restrict__ best_median)
{
    const int i = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (i >= L) return;
    const int lane = threadIdx.x & 63;
    const long long o = off[i], e = off[i + 1];
    const long long nn = e - o;
    if (nn > LM_SMALL) return;                                           // k_landmark_large's
    const int n = __builtin_amdgcn_readfirstlane(nn > 0 ? (int)nn : 0);
    LmDesc mine{{0, 0, 0, 0}};
    if (lane < n) mine = lm_load(desc, o + lane);
    const int k = (n - 1) >> 1;                                          // (size_t)(0.5*(N-1)), N >= 1
    int best = 0, best_med = 0x7fffffff;
    for (int r = 0; r < n; r++) {
        LmDesc row;
        for (int w = 0; w < 4; w++) {
            const unsigned wl = __builtin_amdgcn_readlane((unsigned)mine.w[w], r), wh = __builtin_amdgcn_readlane((unsigned)(mine.w[w] >> 32), r);
            row.w[w] = ((unsigned long long)wh << 32) | wl;
        }
        const int d = lane < n ? lm_dist(row, mine) : 0x7fff;            // lanes beyond N never count
        // smallest v in [0, 256] with count(d <= v) >= k + 1
        int lo = 0, hi = 256;
#pragma unroll
        for (int step = 0; step < 9; step++) {
            const int mid = (lo + hi) >> 1;
            const bool enough = __popcll(__ballot(d <= mid)) > k;
            hi = enough ? mid : hi;
            lo = enough ? lo : mid + 1;
        }
        if (lo < best_med) { best_med = lo; best = r; }
    }
    if (lane == 0) lm_write(i, n, best, best_med, best_idx, best_median);
}

// N > 64: workgroups stride over the batch and take the landmarks the wave path left; wavefront w takes rows w, w + 8, ...
__global__ __launch_bounds__(64 * LM_LARGE_WAVES) void k_landmark_large(const int64_t* __restrict__ off, const uint8_t* __restrict__ desc, int L,
                                                                       int32_t* __restrict__ best_idx, int32_t* __restrict__ best_median)
{
    __shared__ __attribute__((aligned(16))) int hist[LM_LARGE_WAVES][LM_HIST];
    __shared__ unsigned long long wave_key[LM_LARGE_WAVES];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int* h = hist[wv];
    for (int i = blockIdx.x; i < L; i += gridDim.x) {
        const long long o = off[i], nn = off[i + 1] - o;
        if (nn <= LM_SMALL) continue;                                    // block-uniform
        const int n = (int)nn, k = (n - 1) >> 1;
        unsigned long long key = ~0ull;
        for (int r = wv; r < n; r += LM_LARGE_WAVES) {
            reinterpret_cast<int4*>(h)[lane] = make_int4(0, 0, 0, 0);
            if (lane == 0) h[256] = 0;
            LM_WAVE_LDS_SYNC();
            const LmDesc row = lm_load(desc, o + r);
            for (int j = lane; j < n; j += 64) atomicAdd(&h[lm_dist(row, lm_load(desc, o + j))], 1);
            LM_WAVE_LDS_SYNC();
            // lane l owns bins 4l .. 4l+3; the first lane whose inclusive prefix exceeds k holds the median (bin 256 if none does)
            const int4 b = reinterpret_cast<const int4*>(h)[lane];
            const int s = b.x + b.y + b.z + b.w;
            int incl = s;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            const unsigned long long past = __ballot(incl > k);
            int med = 256;
            if (past) {
                const int f = __ffsll((long long)past) - 1;
                int c = incl - s, m = 4 * lane + 3;
                if (c + b.x > k) m = 4 * lane;
                else if (c + b.x + b.y > k) m = 4 * lane + 1;
                else if (c + b.x + b.y + b.z > k) m = 4 * lane + 2;
                med = __shfl(m, f);
            }
            key = min(key, ((unsigned long long)med << 32) | (unsigned)r);
            LM_WAVE_LDS_SYNC();                                          // this row's histogram reads are done before the next row clears it
        }
        if (lane == 0) wave_key[wv] = key;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long m = wave_key[0];
            for (int w = 1; w < LM_LARGE_WAVES; w++) m = min(m, wave_key[w]);
            lm_write(i, n, (int)(m & 0xffffffffu), (int)(m >> 32), best_idx, best_median);
        }
        __syncthreads();                                                 // wave_key is rewritten by the next landmark
    }
}

// any_large = false: the caller knows that no landmark has N > 64 (the host entry point counts them); the large kernel is then not launched
static void launch_landmark_best(const int64_t* d_off, const uint8_t* d_desc, int L, int32_t* d_best, int32_t* d_median, bool any_large, hipStream_t s)
{
    hipLaunchKernelGGL(k_landmark_small, dim3((L + 3) / 4), dim3(256), 0, s, d_off, d_desc, L, d_best, d_median);
    if (any_large) hipLaunchKernelGGL(k_landmark_large, dim3(std::min(L, 2048)), dim3(64 * LM_LARGE_WAVES), 0, s, d_off, d_desc, L, d_best, d_median);
}

// hs_api.hip (as for hs_comm.hip's entry points)
void hs_set_error(hs_orb* h, const char* msg);
int hs_orb_device_of(const hs_orb* h);
hipStream_t hs_orb_stream_of(const hs_orb* h);
uint8_t* hs_orb_scratch_of(hs_orb* h, size_t bytes);

static int lm_fail(hs_orb* h, int code, const char* msg) { hs_set_error(h, msg); return code; }
#define LM_TRY(h, expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { (void)hipGetLastError(); \
    return lm_fail(h, HS_ERR_HIP, hipGetErrorString(e__)); } } while (0)
static size_t lm_pad(size_t b) { return (b + 255) & ~(size_t)255; }

extern "C" {

int hs_landmark_best_descriptors_device(hs_orb* h, const int64_t* d_offsets, const uint8_t* d_desc, int L, int32_t* d_best, int32_t* d_median, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (L < 0 || (L > 0 && (!d_offsets || !d_desc || !d_best || !d_median)) || ((uintptr_t)d_desc & 15) || ((uintptr_t)d_offsets & 7))
        return lm_fail(h, HS_ERR_INVALID, "bad argument");
    if (L == 0) return HS_OK;
    LM_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    launch_landmark_best(d_offsets, d_desc, L, d_best, d_median, true, stream ? (hipStream_t)stream : hs_orb_stream_of(h));
    LM_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_landmark_best_descriptors(hs_orb* h, const int64_t* offsets, const uint8_t* desc, int L, int32_t* best, int32_t* median)
{
    if (!h) return HS_ERR_INVALID;
    if (L < 0 || (L > 0 && (!offsets || !best || !median))) return lm_fail(h, HS_ERR_INVALID, "bad argument");
    if (L == 0) return HS_OK;
    bool any_large = false;
    for (int i = 0; i < L; i++) {
        const int64_t n = offsets[i + 1] - offsets[i];
        if (offsets[i] < 0 || n < 0 || n > INT32_MAX) return lm_fail(h, HS_ERR_INVALID, "offsets must be non-negative and non-decreasing, N < 2^31");
        any_large |= n > LM_SMALL;
    }
    const size_t total = (size_t)offsets[L];
    if (total > 0 && !desc) return lm_fail(h, HS_ERR_INVALID, "bad argument");
    LM_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    const size_t b_off = lm_pad((size_t)(L + 1) * 8), b_desc = lm_pad(std::max(total, (size_t)1) * 32), b_out = lm_pad((size_t)L * 4);
    uint8_t* base = hs_orb_scratch_of(h, b_off + b_desc + 2 * b_out);
    if (!base) return HS_ERR_HIP;
    int64_t* d_off = reinterpret_cast<int64_t*>(base);
    uint8_t* d_desc = base + b_off;
    int32_t* d_best = reinterpret_cast<int32_t*>(base + b_off + b_desc);
    int32_t* d_med = reinterpret_cast<int32_t*>(base + b_off + b_desc + b_out);
    hipStream_t s = hs_orb_stream_of(h);
    LM_TRY(h, hipMemcpyAsync(d_off, offsets, (size_t)(L + 1) * 8, hipMemcpyHostToDevice, s));
    if (total) LM_TRY(h, hipMemcpyAsync(d_desc, desc, total * 32, hipMemcpyHostToDevice, s));
    launch_landmark_best(d_off, d_desc, L, d_best, d_med, any_large, s);
    LM_TRY(h, hipGetLastError());
    LM_TRY(h, hipMemcpyAsync(best, d_best, (size_t)L * 4, hipMemcpyDeviceToHost, s));
    LM_TRY(h, hipMemcpyAsync(median, d_med, (size_t)L * 4, hipMemcpyDeviceToHost, s));
    LM_TRY(h, hipStreamSynchronize(s));
    return HS_OK;
}

}  // extern "C"
