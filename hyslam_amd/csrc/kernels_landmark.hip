// kernels_landmark.hip — a landmark's representative descriptor for a whole batch of landmarks.
//
//   k_landmark_small   MapPointDBEntry::_computeDistinctiveDescriptor_, N <= 64       src/core/MapPointDB.cpp:128-175
//   k_landmark_large   the same, N > 64
//   k_landmark_entries _updateNormalAndDepth_, _updateMeanDistance_, _updateSize_ + the scatter into hs_landmark records   MapPointDB.cpp:230-310
//
// Input is CSR: landmark i owns descriptors desc[off[i] .. off[i+1]) in the caller's order (the reference walks a std::map<KeyFrame*, ...>).
// Row r of the N x N Hamming matrix (diagonal 0 included) has the median element (size_t)(0.5*(N-1)) = (N-1)/2 of its ascending order; the
// reference keeps the first row whose median is strictly smaller than every earlier one.  Distances are integers in [0, 256], so the k-th
// smallest of a row is found by counting, not by sorting:
//   small: one wavefront per landmark, lane j holds descriptor j; per row a 9-step bisection over the value, count(d <= v) by one ballot.
//   large: one workgroup per landmark, one wavefront per row; the row is counted into a 257-bin LDS histogram and the k-th bin read off a
//          wave prefix sum.  LDS does not grow with N, so N is bounded only by memory (and by best[]'s int32).
// Both keep the reference's first-strict-minimum by minimising the key median << 32 | row.
//
// k_landmark_entries: one wavefront per landmark, lane j holds observation base + j of a 64-observation chunk.  The per-observation terms (the
// double cv::norm, 1.0 / norm and its float products, featureSizeMetric) are independent and computed on all lanes; the three float sums depend on
// their order, so they are added strictly left to right: every lane walks the chunk's terms in lane order (readlane) onto a running sum carried
// from the previous chunk.  The rounding of every step is DESIGN.md D8.  It runs after the descriptor kernels on the same stream and reads their
// best[] for the scatter.
#include "hs_match_device.h"
#include <algorithm>
#include <cstring>
#include <vector>

#define LM_SMALL 64            // largest N of the wave path
#define LM_LARGE_WAVES 8       // wavefronts per workgroup of the large path
#define LM_HIST 260            // 257 bins (distance 0..256) rounded up to a multiple of 4: each wave's histogram stays 16-byte aligned

// the wave's earlier LDS accesses are done before its next ones (all lanes): compiler barrier + lgkmcnt(0)
#define LM_WAVE_LDS_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                                __builtin_amdgcn_s_waitcnt(0xc07f); } while (0)

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
    Desc256 mine{{0, 0, 0, 0}};
    if (lane < n) mine = desc_load(desc + (o + lane) * 32);
    const int k = (n - 1) >> 1;                                          // (size_t)(0.5*(N-1)), N >= 1
    int best = 0, best_med = 0x7fffffff;
    for (int r = 0; r < n; r++) {
        Desc256 row;
        for (int w = 0; w < 4; w++) row.w[w] = lane_read(mine.w[w], r);
        const int d = lane < n ? hamming256(row, mine) : 0x7fff;           // lanes beyond N never count
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
            const Desc256 row = desc_load(desc + (o + r) * 32);
            for (int j = lane; j < n; j += 64) atomicAdd(&h[hamming256(row, desc_load(desc + (o + j) * 32))], 1);
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

// cv::norm of a continuous 3 x 1 CV_32F (D8): squares in double, summed left to right, double sqrt; the double is returned
__device__ __forceinline__ double lm_norm3(float a, float b, float c)
{
    double s = __dmul_rn((double)a, (double)a);
    s = __dadd_rn(s, __dmul_rn((double)b, (double)b));
    s = __dadd_rn(s, __dmul_rn((double)c, (double)c));
    return __dsqrt_rn(s);
}

// KeyFrame::featureSizeMetric(idx) (KeyFrame.cc:234-255) with Camera::Unproject (Camera.cpp:155-159)
__device__ __forceinline__ float lm_feature_size(const hs_lm_obs& ob)
{
    if (!ob.assoc) return -1.0f;
    const float z = __double2float_rn(lm_norm3(__fsub_rn(ob.assoc_pos[0], ob.Ow[0]), __fsub_rn(ob.assoc_pos[1], ob.Ow[1]),
                                               __fsub_rn(ob.assoc_pos[2], ob.Ow[2])));
    if (z < 0.0f) return -1.0f;                                          // as written (:243); a norm is never negative
    const float r = __fdiv_rn(ob.kp_size, 2.0f);
    const float zx = __fdiv_rn(z, ob.fx), zy = __fdiv_rn(z, ob.fy);
    const float xl = __fmul_rn(__fsub_rn(__fsub_rn(ob.u, r), ob.cx), zx), yl = __fmul_rn(__fsub_rn(ob.v, ob.cy), zy);
    const float xr = __fmul_rn(__fsub_rn(__fadd_rn(ob.u, r), ob.cx), zx), yr = __fmul_rn(__fsub_rn(ob.v, ob.cy), zy);
    return __double2float_rn(lm_norm3(__fsub_rn(xr, xl), __fsub_rn(yr, yl), __fsub_rn(z, z)));
}

struct LmEntryArgs {
    hs_lm_entry_params prm;
    int L;
    const hs_lm_entry_in* entries;
    const int64_t* obs_off;
    const hs_lm_obs* obs;
    const int64_t* desc_off;
    const uint8_t* desc;
    const int32_t* best;                 // the descriptor kernels' output
    float *normal, *min_dist, *max_dist, *mean_dist, *size;
    int32_t* flags;
    hs_landmark* lms;                    // scatter target, nullptr = none
    const int32_t* lm_index;
    int n_lms;
};

// four landmarks per 256-thread block, one per wavefront
__global__ __launch_bounds__(256) void k_landmark_entries(LmEntryArgs a)
{
    const int i = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (i >= a.L) return;
    const int lane = threadIdx.x & 63;
    const long long o = a.obs_off[i];
    const long long n = __builtin_amdgcn_readfirstlane(a.obs_off[i + 1] - o);
    const hs_lm_entry_in e = a.entries[i];
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, mean = 0.0f, size = 0.0f;    // normal = cv::Mat::zeros (:244), mean_dist = 0.0, mean_size = 0.0
    long long npos = 0;
    for (long long base = 0; base < n; base += 64) {
        const int cnt = (int)min(64LL, n - base);
        float tx = 0.0f, ty = 0.0f, tz = 0.0f, dist = 0.0f, sz = -1.0f;
        if (lane < cnt) {
            const hs_lm_obs ob = a.obs[o + base + lane];
            const float dx = __fsub_rn(e.pos[0], ob.Ow[0]), dy = __fsub_rn(e.pos[1], ob.Ow[1]), dz = __fsub_rn(e.pos[2], ob.Ow[2]);
            const double s = lm_norm3(dx, dy, dz);
            const float alpha = __double2float_rn(__ddiv_rn(1.0, s));   // normali / cv::norm(normali): alpha = 1.0/s, scaleAdd rounds it to float
            tx = __fmul_rn(dx, alpha); ty = __fmul_rn(dy, alpha); tz = __fmul_rn(dz, alpha);
            dist = __double2float_rn(s);                                // float this_dist = cv::norm(Pos_cam) (:282)
            sz = lm_feature_size(ob);
        }
        for (int j = 0; j < cnt; j++) {                                 // observation order; never a tree
            nx = __fadd_rn(lane_read(tx, j), nx); ny = __fadd_rn(lane_read(ty, j), ny); nz = __fadd_rn(lane_read(tz, j), nz);
            mean = __fadd_rn(mean, lane_read(dist, j));
            const float sj = lane_read(sz, j);
            if (sj > 0.0f) { size = __fadd_rn(size, sj); npos++; }      // (:298-301)
        }
    }
    const bool has = n > 0;
    // normal / n = convertTo(alpha = 1.0/n, beta = 0): fl(fl(x * (float)alpha) + 0.0f) (D8)
    const float an = has ? __double2float_rn(__ddiv_rn(1.0, (double)(int)n)) : 0.0f;
    nx = __fadd_rn(__fmul_rn(nx, an), 0.0f); ny = __fadd_rn(__fmul_rn(ny, an), 0.0f); nz = __fadd_rn(__fmul_rn(nz, an), 0.0f);
    const float dref = __double2float_rn(lm_norm3(__fsub_rn(e.pos[0], e.ref_Ow[0]), __fsub_rn(e.pos[1], e.ref_Ow[1]), __fsub_rn(e.pos[2], e.ref_Ow[2])));
    const float maxd = __fmul_rn(a.prm.max_dist_factor, dref), mind = __fmul_rn(a.prm.min_dist_factor, dref);
    mean = __fdiv_rn(mean, (float)(int)n);
    size = __fdiv_rn(size, (float)(int)npos);                           // 0.0f / 0.0f = NaN without a positive size (no early return)
    const int best = a.best[i];
    if (lane == 0) {
        if (has) {
            a.normal[3LL * i] = nx; a.normal[3LL * i + 1] = ny; a.normal[3LL * i + 2] = nz;
            a.min_dist[i] = mind; a.max_dist[i] = maxd; a.mean_dist[i] = mean;
        }
        a.size[i] = size;
        a.flags[i] = (has ? HS_LM_SET_NORMAL_DEPTH | HS_LM_SET_MEAN : 0) | (best >= 0 ? HS_LM_SET_DESC : 0) | HS_LM_SET_SIZE;
    }
    if (!a.lms) return;
    const int t = a.lm_index[i];
    if (t < 0 || t >= a.n_lms) return;
    hs_landmark* r = a.lms + t;                                          // pos, assoc_kp, prev_angle, skip: never written
    if (lane == 0) {
        if (has) { r->normal[0] = nx; r->normal[1] = ny; r->normal[2] = nz; r->min_dist = mind; r->max_dist = maxd; }
        r->size = size;
    }
    if (best >= 0 && lane < 8) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.desc + (a.desc_off[i] + best) * 32);
        reinterpret_cast<uint32_t*>(r->desc)[lane] = src[lane];
    }
}

extern "C" {

int hs_landmark_best_descriptors_device(hs_orb* h, const int64_t* d_offsets, const uint8_t* d_desc, int L, int32_t* d_best, int32_t* d_median, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (L < 0 || (L > 0 && (!d_offsets || !d_desc || !d_best || !d_median)) || ((uintptr_t)d_desc & 15) || ((uintptr_t)d_offsets & 7))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (L == 0) return HS_OK;
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    launch_landmark_best(d_offsets, d_desc, L, d_best, d_median, true, hs_stream_or(h, stream));
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

static int lm_check_csr(hs_orb* h, const int64_t* off, int L, bool* any_large)
{
    for (int i = 0; i < L; i++) {
        const int64_t n = off[i + 1] - off[i];
        if (off[i] < 0 || n < 0 || n > INT32_MAX) return hs_fail(h, HS_ERR_INVALID, "offsets must be non-negative and non-decreasing, N < 2^31");
        if (any_large) *any_large |= n > LM_SMALL;
    }
    return HS_OK;
}

int hs_landmark_best_descriptors(hs_orb* h, const int64_t* offsets, const uint8_t* desc, int L, int32_t* best, int32_t* median)
{
    if (!h) return HS_ERR_INVALID;
    if (L < 0 || (L > 0 && (!offsets || !best || !median))) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (L == 0) return HS_OK;
    bool any_large = false;
    int rc = lm_check_csr(h, offsets, L, &any_large);
    if (rc != HS_OK) return rc;
    const size_t total = (size_t)offsets[L];
    if (total > 0 && !desc) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    HsStage st(h);
    int64_t* d_off; uint8_t* d_desc; int32_t *d_best, *d_med;
    st.in(&d_off, (size_t)L + 1, offsets); st.in(&d_desc, total * 32, desc); st.out(&d_best, L, best); st.out(&d_med, L, median);
    rc = st.begin();
    if (rc != HS_OK) return rc;
    launch_landmark_best(d_off, d_desc, L, d_best, d_med, any_large, st.stream());
    return st.finish();
}

int hs_landmark_update_entries_device(hs_orb* h, const hs_lm_entry_params* params, int L, const hs_lm_entry_in* d_entries,
                                      const int64_t* d_obs_offsets, const hs_lm_obs* d_obs, const int64_t* d_desc_offsets, const uint8_t* d_desc,
                                      float* d_normal, float* d_min_dist, float* d_max_dist, float* d_mean_dist, float* d_size,
                                      int32_t* d_best, int32_t* d_median, int32_t* d_flags,
                                      hs_landmark* d_lms, const int32_t* d_lm_index, int n_lms, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!params || L < 0 || n_lms < 0 || (d_lms == nullptr) != (d_lm_index == nullptr)) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (L == 0) return HS_OK;
    if (!d_entries || !d_obs_offsets || !d_obs || !d_desc_offsets || !d_desc || !d_normal || !d_min_dist || !d_max_dist || !d_mean_dist || !d_size ||
        !d_best || !d_median || !d_flags || ((uintptr_t)d_desc & 15) || ((uintptr_t)d_obs_offsets & 7) || ((uintptr_t)d_desc_offsets & 7) ||
        ((uintptr_t)d_entries & 3) || ((uintptr_t)d_obs & 3) || ((uintptr_t)d_lms & 3) || ((uintptr_t)d_lm_index & 3))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    const hipStream_t s = hs_stream_or(h, stream);
    const LmEntryArgs a{*params, L, d_entries, d_obs_offsets, d_obs, d_desc_offsets, d_desc, d_best,
                        d_normal, d_min_dist, d_max_dist, d_mean_dist, d_size, d_flags, d_lms, d_lm_index, n_lms};
    launch_landmark_best(d_desc_offsets, d_desc, L, d_best, d_median, true, s);
    hipLaunchKernelGGL(k_landmark_entries, dim3((L + 3) / 4), dim3(256), 0, s, a);
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_landmark_update_entries(hs_orb* h, const hs_lm_entry_params* params, int L, const hs_lm_entry_in* entries,
                               const int64_t* obs_offsets, const hs_lm_obs* obs, const int64_t* desc_offsets, const uint8_t* desc,
                               float* out_normal, float* out_min_dist, float* out_max_dist, float* out_mean_dist, float* out_size,
                               int32_t* out_best, int32_t* out_median, int32_t* out_flags)
{
    if (!h) return HS_ERR_INVALID;
    if (!params || L < 0) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (L == 0) return HS_OK;
    if (!entries || !obs_offsets || !desc_offsets || !out_normal || !out_min_dist || !out_max_dist || !out_mean_dist || !out_size || !out_best ||
        !out_median || !out_flags)
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    bool any_large = false;
    int st = lm_check_csr(h, obs_offsets, L, nullptr);
    if (st == HS_OK) st = lm_check_csr(h, desc_offsets, L, &any_large);
    if (st != HS_OK) return st;
    const size_t n_obs = (size_t)obs_offsets[L], n_desc = (size_t)desc_offsets[L];
    if ((n_obs > 0 && !obs) || (n_desc > 0 && !desc)) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    // the outputs the reference leaves unchanged for N = 0 come back through a host copy and are merged by flag
    std::vector<float> nrm((size_t)L * 3), f3((size_t)L * 3);
    HsStage stg(h);
    hs_lm_entry_in* d_ent; int64_t *d_ooff, *d_doff; hs_lm_obs* d_obs; uint8_t* d_desc; float *d_normal, *d_f[4]; int32_t* d_i[3];
    stg.in(&d_ent, L, entries); stg.in(&d_ooff, (size_t)L + 1, obs_offsets); stg.in(&d_doff, (size_t)L + 1, desc_offsets);
    stg.in(&d_obs, n_obs, obs); stg.in(&d_desc, n_desc * 32, desc);
    stg.out(&d_normal, (size_t)L * 3, nrm.data());
    for (int k = 0; k < 3; k++) stg.out(&d_f[k], L, f3.data() + (size_t)k * L);       // min_dist, max_dist, mean_dist
    stg.out(&d_f[3], L, out_size);
    stg.out(&d_i[0], L, out_best); stg.out(&d_i[1], L, out_median); stg.out(&d_i[2], L, out_flags);
    st = stg.begin();
    if (st != HS_OK) return st;
    const hipStream_t s = stg.stream();
    const LmEntryArgs a{*params, L, d_ent, d_ooff, d_obs, d_doff, d_desc, d_i[0],
                        d_normal, d_f[0], d_f[1], d_f[2], d_f[3], d_i[2], nullptr, nullptr, 0};
    launch_landmark_best(d_doff, d_desc, L, d_i[0], d_i[1], any_large, s);
    hipLaunchKernelGGL(k_landmark_entries, dim3((L + 3) / 4), dim3(256), 0, s, a);
    st = stg.finish();
    if (st != HS_OK) return st;
    for (int i = 0; i < L; i++) {
        if (!(out_flags[i] & HS_LM_SET_NORMAL_DEPTH)) continue;
        std::memcpy(out_normal + 3 * (size_t)i, nrm.data() + 3 * (size_t)i, 12);
        out_min_dist[i] = f3[i]; out_max_dist[i] = f3[(size_t)L + i]; out_mean_dist[i] = f3[2 * (size_t)L + i];
    }
    return HS_OK;
}

}  // extern "C"
