// kernels_stereo.hip — K8a: left<->right stereo matching by Hamming distance.
//
// Replaces Stereomatcher::computeStereoMatches (src/features/Stereomatcher.cpp:36-156) and the
// ORBDistance bit-hack it calls per pair (src/features/low_level/DescriptorDistance.cpp:9-25).
// The reference builds a per-row table of right keypoints (iR listed in rows floor(y-r)..ceil(y+r),
// r = 2*size/size_ref) and scans vRowIndices[(int)vL] in ascending iR.  Here the right keypoints are binned once per pair into 32-row
// STRIPS (k_stereo_strips: the reference's table at 1/32 of its size); one wavefront owns one left keypoint, scans the strip of its row
// (~100 candidates instead of all 2000) and re-applies the exact predicate (row band, |octave diff| <= 1, uL-maxD <= uR <= uL) to every
// candidate.  The running minimum uses the key dist<<16 | iR, which reproduces the reference's strict `dist < bestDist` over ascending iR
// (first minimum wins) whatever the order inside a strip.  Descriptors are XORed as 4 x u64 and counted with v_bcnt (__popcll) — equal
// to the reference's 32-bit parallel bit count.
//
// Second kernel: the reference's sort + median + 2.1*median rejection (:142-155) is a histogram of the
// accepted integer distances, one workgroup per pair.
// Documented deviation D2 (reference UB): rows outside [0,nRows) are ignored, no match => no filtering.
// A left keypoint whose row has candidates but none closer than TH_HIGH keeps the reference's initial bestDist = TH_HIGH, bestIdxR = 0
// (:92-93): with TH_LOW > TH_HIGH that passes the acceptance test and pairs it with right keypoint 0.  Its distance is stored as
// SM_DIST_TH_HIGH, which sorts after every real distance (all of them are below TH_HIGH) in the median's histogram.
#define SM_DIST_TH_HIGH 257
#include "hs_internal.h"
#include "hs_stereo.h"

// Right keypoints binned into 32-row strips once per pair: a right keypoint lists itself in every strip its row band
// [floor(y-r), ceil(y+r)] touches (1-2 strips), so a left keypoint at row v only scans strip v>>5 — ~100 candidates instead of all
// 2000 (the reference's per-row table, Stereomatcher.cpp:46-63, at 1/32 of its size).  The exact band test is repeated per candidate.
#define STRIP_SHIFT HS_STRIP_SHIFT

// One workgroup per pair: the strip counters live in LDS (a slot is an LDS atomic away, not a round trip to L2), every right keypoint's
// record is loaded up front, and the counters are written out whole, so nothing has to be zeroed between calls.
#define STRIPS_T 1024
#define STRIPS_MAX HS_STRIPS_MAX   // 65536 rows / 32 (HsStripEntry: hs_internal.h)
__global__ __launch_bounds__(STRIPS_T) void k_stereo_strips(const hs_keypoint* __restrict__ kpsR, const int32_t* __restrict__ nRs, int cap,
                                                            float size_ref, int n_rows, int n_strips,
                                                            int32_t* __restrict__ strip_count, HsStripEntry* __restrict__ strip_list)
{
    __shared__ int s_cnt[STRIPS_MAX];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int nR = min(nRs[pair], cap);
    for (int s = tid; s < n_strips; s += STRIPS_T) s_cnt[s] = 0;
    constexpr int KPT = 4;                                    // keypoints per thread whose records are in flight together
    __syncthreads();
    for (int i0 = 0; i0 < nR; i0 += STRIPS_T * KPT) {
        float kx[KPT], ky[KPT], ks[KPT]; int ko[KPT];
#pragma unroll
        for (int k = 0; k < KPT; k++) {
            const int i = min(i0 + tid + STRIPS_T * k, nR - 1);
            const hs_keypoint* kr = &kpsR[(size_t)pair * cap + i];
            kx[k] = kr->x; ky[k] = kr->y; ks[k] = kr->size; ko[k] = kr->octave;
        }
#pragma unroll
        for (int k = 0; k < KPT; k++) {
            const int i = i0 + tid + STRIPS_T * k;
            if (i >= nR) continue;
            const float r = 2.0f * ks[k] / size_ref;         // :56
            int maxr = (int)ceilf(ky[k] + r), minr = (int)floorf(ky[k] - r);
            if (maxr < 0 || minr >= n_rows) continue;         // rows outside [0, nRows) do not exist (D2)
            minr = max(minr, 0); maxr = min(maxr, n_rows - 1);
            for (int s = minr >> STRIP_SHIFT; s <= (maxr >> STRIP_SHIFT); s++) {
                const int slot = atomicAdd(&s_cnt[s], 1);
                const int lo = max(minr - (s << STRIP_SHIFT), 0), hi = min(maxr - (s << STRIP_SHIFT), 31);
                HsStripEntry e; e.uR = kx[k]; e.octave = ko[k]; e.idx_band = (uint32_t)i | ((uint32_t)lo << 16) | ((uint32_t)hi << 24); e._pad = 0;
                strip_list[((size_t)pair * n_strips + s) * cap + slot] = e;
            }
        }
    }
    __syncthreads();
    for (int s = tid; s < n_strips; s += STRIPS_T) strip_count[(size_t)pair * n_strips + s] = s_cnt[s];
}

// One wavefront owns TWO left keypoints and walks both strips together (the kernel is a chain of dependent loads — strip entry, then the
// descriptors of the candidates that pass — and nothing else: twice the loads in flight per wave, half the waves).
// (Counters at 64 pairs per call: 0.72 VALU per busy CU cycle, issue-bound, not latency-bound — large batches run k_stereo_match_compact below;
// <1> is the instance of small calls, <2> a tuning / parity variant: hs_stereo_kpw.)
template <int SM_KPW>              // left keypoints per wavefront: 2, or 1 when the launch has too few workgroups to fill the chip anyway (single pairs)
__global__ __launch_bounds__(256) void k_stereo_match(const int32_t* __restrict__ strip_count, const HsStripEntry* __restrict__ strip_list, int n_strips,
                                                      const hs_keypoint* __restrict__ kpsL, const uint8_t* __restrict__ descL,
                                                      const int32_t* __restrict__ nLs,
                                                      const hs_keypoint* __restrict__ kpsR, const uint8_t* __restrict__ descR,
                                                      const int32_t* __restrict__ nRs,
                                                      int cap, hs_stereo_params sp,
                                                      float* __restrict__ uRight, float* __restrict__ depth, int32_t* __restrict__ best_dist)
{
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform: the left keypoints' records come through scalar loads
    const int pair = blockIdx.y;
    const int iL0 = (blockIdx.x * 4 + wv) * SM_KPW;
    const int nL = min(nLs[pair], cap);
    if (iL0 >= cap) return;
    const size_t o = (size_t)pair * cap;
    const float mbf = sp.mbf, mb = sp.mbf / sp.fx;
    const float minD = 0.f, maxD = mbf / mb;                 // :66-68
    const float th_high = sp.th_high;

    float uL[SM_KPW], minU[SM_KPW], maxU[SM_KPW]; int levelL[SM_KPW], rowIn[SM_KPW], nc[SM_KPW];
    const HsStripEntry* cl[SM_KPW]; const unsigned long long* dl[SM_KPW];
    bool live[SM_KPW];
    int ncmax = 0;
#pragma unroll
    for (int t = 0; t < SM_KPW; t++) {
        const int iL = iL0 + t;
        live[t] = iL < nL;
        const hs_keypoint kl = kpsL[o + min(iL, max(nL - 1, 0))];
        const float vL = kl.y;
        uL[t] = kl.x; levelL[t] = kl.octave;
        minU[t] = uL[t] - maxD; maxU[t] = uL[t] - minD;
        const int rowL = (int)vL;                             // vRowIndices[vL]
        const bool ok = live[t] && (vL >= 0.f) && rowL < sp.n_rows && !(maxU[t] < 0.f);
        const size_t sb = (size_t)pair * n_strips + (ok ? (rowL >> STRIP_SHIFT) : 0);
        nc[t] = ok ? strip_count[sb] : 0;
        cl[t] = strip_list + sb * cap;
        rowIn[t] = rowL & 31;
        dl[t] = reinterpret_cast<const unsigned long long*>(descL + (o + min(iL, max(nL - 1, 0))) * 32);
        ncmax = max(ncmax, nc[t]);
    }
    // bestDist starts at TH_HIGH and only strictly smaller distances replace it (:92,114)
    uint32_t best[SM_KPW];
#pragma unroll
    for (int t = 0; t < SM_KPW; t++) best[t] = 0xFFFFFFFFu;
    // two candidates per lane, keypoint and round (a strip holds ~100).  Lanes without a candidate re-read the strip's first entry and are masked.
    for (int c0 = 0; c0 < ncmax; c0 += 128) {
        HsStripEntry e[SM_KPW][2]; bool pass[SM_KPW][2];
#pragma unroll
        for (int t = 0; t < SM_KPW; t++)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int c = c0 + 64 * j + lane;
                pass[t][j] = c < nc[t];
                e[t][j] = cl[t][pass[t][j] ? c : 0];
            }
#pragma unroll
        for (int t = 0; t < SM_KPW; t++)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int lo = (int)((e[t][j].idx_band >> 16) & 0xFFu), hi = (int)(e[t][j].idx_band >> 24);
                pass[t][j] = pass[t][j] && !(rowIn[t] < lo || rowIn[t] > hi);
                pass[t][j] = pass[t][j] && !(e[t][j].octave < levelL[t] - 1 || e[t][j].octave > levelL[t] + 1);
                pass[t][j] = pass[t][j] && (e[t][j].uR >= minU[t] && e[t][j].uR <= maxU[t]);
            }
        unsigned long long dr[SM_KPW][2][4];                  // descriptors only of the candidates that passed (a fifth of them)
#pragma unroll
        for (int t = 0; t < SM_KPW; t++)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const unsigned long long* p = reinterpret_cast<const unsigned long long*>(descR + (o + (e[t][j].idx_band & 0xFFFFu)) * 32);
                if (pass[t][j]) { dr[t][j][0] = p[0]; dr[t][j][1] = p[1]; dr[t][j][2] = p[2]; dr[t][j][3] = p[3]; }
                else { dr[t][j][0] = dr[t][j][1] = dr[t][j][2] = dr[t][j][3] = 0ull; }
            }
#pragma unroll
        for (int t = 0; t < SM_KPW; t++) {
            const unsigned long long l0 = dl[t][0], l1 = dl[t][1], l2 = dl[t][2], l3 = dl[t][3];      // uniform: scalar loads
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int d = __popcll(l0 ^ dr[t][j][0]) + __popcll(l1 ^ dr[t][j][1]) + __popcll(l2 ^ dr[t][j][2]) + __popcll(l3 ^ dr[t][j][3]);
                if (pass[t][j] && (float)d < th_high) best[t] = min(best[t], ((uint32_t)d << 16) | (e[t][j].idx_band & 0xFFFFu));
            }
        }
    }
#pragma unroll
    for (int t = 0; t < SM_KPW; t++) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) best[t] = min(best[t], (uint32_t)__shfl_xor((int)best[t], s, 64));
        // nothing beat TH_HIGH: bestDist = TH_HIGH stands, and is accepted when TH_HIGH < (TH_HIGH + TH_LOW) / 2 — only if the row has any
        // candidate at all (vRowIndices[vL] not empty, :84).  Wave-uniform and rare (TH_LOW > TH_HIGH), so the strip is scanned again here
        // rather than tracked in the loop above.
        bool rowHasCandidates = false;
        if (best[t] == 0xFFFFFFFFu && sp.th_high < (sp.th_high + sp.th_low) / 2) {
            bool hit = false;
            for (int c = lane; c < nc[t]; c += 64) {
                const uint32_t ib = cl[t][c].idx_band;
                hit = hit || !(rowIn[t] < (int)((ib >> 16) & 0xFFu) || rowIn[t] > (int)(ib >> 24));
            }
            rowHasCandidates = __ballot(hit) != 0ull;
        }
        const int iL = iL0 + t;
        if (iL >= cap) break;
        if (lane == 0) {
            float ur_out = -1.0f, depth_out = -1.0f; int bd = -1;
            if (live[t] && (best[t] != 0xFFFFFFFFu || rowHasCandidates)) {
                const bool found = best[t] != 0xFFFFFFFFu;
                const float bestDist = found ? (float)(best[t] >> 16) : th_high;                // :92-93 when nothing beat TH_HIGH
                const int bestIdxR = found ? (int)(best[t] & 0xFFFF) : 0;
                const float dist_threshold = (sp.th_high + sp.th_low) / 2;          // :41
                if (bestDist < dist_threshold) {
                    float uR0 = kpsR[o + bestIdxR].x;
                    float disparity = uL[t] - uR0;
                    if (disparity >= minD && disparity < maxD) {
                        if (disparity <= 0) { disparity = 0.01; uR0 = uL[t] - 0.01; }    // double constants, as in the reference (:130-131)
                        depth_out = mbf / disparity;
                        ur_out = uR0;
                        bd = found ? (int)(best[t] >> 16) : SM_DIST_TH_HIGH;
                    }
                }
            }
            uRight[o + iL] = ur_out; depth[o + iL] = depth_out; best_dist[o + iL] = bd;
        }
    }
}

// Large batches: the same walk with the Hamming part on DENSE lanes.  At two keypoints per wave the kernel is issue-bound (0.72 VALU per busy CU
// cycle), and most of what it issues is the descriptor part of k_stereo_match — four 8-byte loads, 8 v_xor, 8 v_bcnt, the adds and the key minimum —
// on slots whose candidate failed the gate.  Here a wave owns K left keypoints (their records live in lanes 0 .. K-1, so the fixed part — record
// loads, reduction, epilogue — is paid once per K) and works in two alternating steps:
//   gate     two strip entries per lane and round of one keypoint, the predicate of k_stereo_match with its expressions; what passes is appended
//            as t << 16 | iR to the wave's queue in LDS (ballot + mbcnt).  The band test alone is kept per keypoint in a mask: rowHasCandidates.
//   Hamming  as soon as the queue holds 64 entries its LAST 64 are taken off, one per lane (the order of candidates does not matter: the key
//            d << 16 | iR is a first-minimum-wins whatever order they come in), the minimum per keypoint with an LDS atomicMin on K slots — only
//            the lanes under TH_HIGH get that far.  A gate round adds at most 128 entries to at most 63: SMC_QCAP.  The rest goes out at the end.
// One wave's LDS instructions execute in issue order, so its lanes hand data to each other through LDS without a barrier; SMC_FENCE keeps the
// compiler from moving an LDS access over a hand-over point.
#define SMC_QCAP 192
#define SMC_FENCE() __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront")
__device__ __forceinline__ int smc_wave_append(bool flag, int& base)
{
    const unsigned long long m = __ballot(flag);
    const int slot = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    base += (int)__popcll(m);
    return slot;
}
template <int K>                   // left keypoints per wavefront: 4 or 8
__global__ __launch_bounds__(256) void k_stereo_match_compact(const int32_t* __restrict__ strip_count, const HsStripEntry* __restrict__ strip_list, int n_strips,
                                                              const hs_keypoint* __restrict__ kpsL, const uint8_t* __restrict__ descL,
                                                              const int32_t* __restrict__ nLs,
                                                              const hs_keypoint* __restrict__ kpsR, const uint8_t* __restrict__ descR,
                                                              const int32_t* __restrict__ nRs,
                                                              int cap, hs_stereo_params sp,
                                                              float* __restrict__ uRight, float* __restrict__ depth, int32_t* __restrict__ best_dist)
{
    static_assert(K >= 2 && K <= 16 && (K & (K - 1)) == 0, "K keypoint records and 4 K descriptor words fit the lanes of a wave");
    __shared__ uint32_t s_queue[4][SMC_QCAP];
    __shared__ __attribute__((aligned(16))) unsigned long long s_descL[4][K][4];
    __shared__ uint32_t s_best[4][K];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pair = blockIdx.y;
    const int iL0 = (blockIdx.x * 4 + wv) * K;
    if (iL0 >= cap) return;                                  // (whole waves: the kernel has no workgroup barrier)
    const int nL = min(nLs[pair], cap);
    const size_t o = (size_t)pair * cap;
    const float mbf = sp.mbf, mb = sp.mbf / sp.fx;
    const float minD = 0.f, maxD = mbf / mb;                 // :66-68
    const float th_high = sp.th_high;
    uint32_t* const queue = s_queue[wv];

    // lane t < K holds the record of left keypoint iL0 + t (the other lanes repeat the last one), as k_stereo_match computes it
    const int iL = iL0 + min(lane, K - 1);
    const bool live = iL < nL;
    const hs_keypoint kl = kpsL[o + min(iL, max(nL - 1, 0))];
    const float vL = kl.y, uL = kl.x;
    const int levelL = kl.octave;
    const float minU = uL - maxD, maxU = uL - minD;
    const int rowL = (int)vL;                                 // vRowIndices[vL]
    const bool ok = live && (vL >= 0.f) && rowL < sp.n_rows && !(maxU < 0.f);
    const int sb = pair * n_strips + (ok ? (rowL >> STRIP_SHIFT) : 0);
    const int nc = ok ? strip_count[sb] : 0;
    const int rowIn = rowL & 31;
    if (lane < 4 * K) {                                       // the K left descriptors: one 8-byte word per lane
        const int il = iL0 + (lane >> 2);
        s_descL[wv][lane >> 2][lane & 3] = reinterpret_cast<const unsigned long long*>(descL + (o + min(il, max(nL - 1, 0))) * 32)[lane & 3];
    }
    if (lane < K) s_best[wv][lane] = 0xFFFFFFFFu;             // bestDist starts at TH_HIGH and only strictly smaller distances replace it (:92,114)
    SMC_FENCE();

    // one queue entry per lane: the distance to the entry's right descriptor, the minimum of its keypoint
    auto hamming = [&](int qi, bool act) {
        const uint32_t q = act ? queue[qi] : 0u;
        const int tq = (int)(q >> 16), iR = (int)(q & 0xFFFFu);
        if (act) {
            const unsigned long long* p = reinterpret_cast<const unsigned long long*>(descR + (o + iR) * 32);
            const unsigned long long r0 = p[0], r1 = p[1], r2 = p[2], r3 = p[3];
            const ulonglong2 la = *reinterpret_cast<const ulonglong2*>(&s_descL[wv][tq][0]), lb = *reinterpret_cast<const ulonglong2*>(&s_descL[wv][tq][2]);
            const int d = __popcll(la.x ^ r0) + __popcll(la.y ^ r1) + __popcll(lb.x ^ r2) + __popcll(lb.y ^ r3);
            if ((float)d < th_high) atomicMin(&s_best[wv][tq], ((uint32_t)d << 16) | (uint32_t)iR);
        }
    };

    int qn = 0;                                               // entries in the queue (wave-uniform)
    uint32_t band_mask = 0;                                   // bit t: an entry of keypoint t's strip has the keypoint's row in its band
#pragma nounroll
    for (int t = 0; t < K; t++) {
        const int nc_t = __builtin_amdgcn_readlane(nc, t);
        if (nc_t == 0) continue;
        const HsStripEntry* const cl = strip_list + (size_t)__builtin_amdgcn_readlane(sb, t) * cap;
        const int rowIn_t = __builtin_amdgcn_readlane(rowIn, t), levelL_t = __builtin_amdgcn_readlane(levelL, t);
        const float minU_t = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(minU), t));
        const float maxU_t = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(maxU), t));
        for (int c0 = 0; c0 < nc_t; c0 += 128) {
            HsStripEntry e[2]; bool band[2], pass[2];
#pragma unroll
            for (int j = 0; j < 2; j++) {                     // lanes without a candidate re-read the strip's first entry and are masked
                const int c = c0 + 64 * j + lane;
                band[j] = c < nc_t;
                e[j] = cl[band[j] ? c : 0];
            }
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int lo = (int)((e[j].idx_band >> 16) & 0xFFu), hi = (int)(e[j].idx_band >> 24);
                band[j] = band[j] && !(rowIn_t < lo || rowIn_t > hi);
                pass[j] = band[j] && !(e[j].octave < levelL_t - 1 || e[j].octave > levelL_t + 1);
                pass[j] = pass[j] && (e[j].uR >= minU_t && e[j].uR <= maxU_t);
            }
            if (__ballot(band[0] || band[1]) != 0ull) band_mask |= 1u << t;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int slot = smc_wave_append(pass[j], qn);
                if (pass[j]) queue[slot] = ((uint32_t)t << 16) | (e[j].idx_band & 0xFFFFu);
            }
            SMC_FENCE();
            while (qn >= 64) { qn -= 64; hamming(qn + lane, true); }
            SMC_FENCE();
        }
    }
    if (qn > 0) hamming(lane, lane < qn);
    SMC_FENCE();

    // lane t finishes keypoint t: the statements of k_stereo_match's epilogue
    if (lane < K && iL < cap) {
        const uint32_t best = s_best[wv][lane];
        // nothing beat TH_HIGH: bestDist = TH_HIGH stands, and is accepted when TH_HIGH < (TH_HIGH + TH_LOW) / 2 — only if the row has any
        // candidate at all (vRowIndices[vL] not empty, :84)
        const bool rowHasCandidates = best == 0xFFFFFFFFu && sp.th_high < (sp.th_high + sp.th_low) / 2 && ((band_mask >> lane) & 1u) != 0;
        float ur_out = -1.0f, depth_out = -1.0f; int bd = -1;
        if (live && (best != 0xFFFFFFFFu || rowHasCandidates)) {
            const bool found = best != 0xFFFFFFFFu;
            const float bestDist = found ? (float)(best >> 16) : th_high;                // :92-93 when nothing beat TH_HIGH
            const int bestIdxR = found ? (int)(best & 0xFFFF) : 0;
            const float dist_threshold = (sp.th_high + sp.th_low) / 2;          // :41
            if (bestDist < dist_threshold) {
                float uR0 = kpsR[o + bestIdxR].x;
                float disparity = uL - uR0;
                if (disparity >= minD && disparity < maxD) {
                    if (disparity <= 0) { disparity = 0.01; uR0 = uL - 0.01; }    // double constants, as in the reference (:130-131)
                    depth_out = mbf / disparity;
                    ur_out = uR0;
                    bd = found ? (int)(best >> 16) : SM_DIST_TH_HIGH;
                }
            }
        }
        uRight[o + iL] = ur_out; depth[o + iL] = depth_out; best_dist[o + iL] = bd;
    }
}

__global__ __launch_bounds__(256) void k_stereo_median(const int32_t* __restrict__ nLs, int cap,
                                                       float* __restrict__ uRight, float* __restrict__ depth,
                                                       const int32_t* __restrict__ best_dist, float th_high,
                                                       int32_t* __restrict__ strip_count, int n_strips)
{
    __shared__ int hist[258];                                 // distances 0..256, then SM_DIST_TH_HIGH (a distance of TH_HIGH, above all others)
    __shared__ float s_th;
    const int pair = blockIdx.x;
    const int nL = min(nLs[pair], cap);
    const size_t o = (size_t)pair * cap;
    for (int i = threadIdx.x; i < 258; i += 256) hist[i] = 0;
    __syncthreads();
    // the distances stay in registers between the histogram and the rejection sweep (8 per thread cover cap <= 2048; more loop again below)
    constexpr int DPT = 8;
    int dreg[DPT];
#pragma unroll
    for (int k = 0; k < DPT; k++) { const int i = threadIdx.x + 256 * k; dreg[k] = i < nL ? best_dist[o + i] : -1; }
#pragma unroll
    for (int k = 0; k < DPT; k++) if (dreg[k] >= 0) atomicAdd(&hist[min(dreg[k], 257)], 1);
    for (int i = threadIdx.x + 256 * DPT; i < nL; i += 256) {
        int d = best_dist[o + i];
        if (d >= 0) atomicAdd(&hist[min(d, 257)], 1);
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        // sorted (dist, iL) pairs: element total/2 carries the median distance (:142-144) = the first bin at which the running count exceeds
        // total/2.  One wavefront: four bins per lane (+ bins 256, 257), inclusive scan over the lanes, the crossing lane finishes inside its bins.
        const int lane = threadIdx.x;
        const int b0 = hist[4 * lane], b1 = hist[4 * lane + 1], b2 = hist[4 * lane + 2], b3 = hist[4 * lane + 3];
        int incl = b0 + b1 + b2 + b3;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) { const int v = __shfl_up(incl, s, 64); if (lane >= s) incl += v; }
        const int below256 = __shfl(incl, 63, 64), total = below256 + hist[256] + hist[257];
        const int target = total / 2, excl = incl - (b0 + b1 + b2 + b3);
        int med = -1;
        if (excl <= target && incl > target) med = 4 * lane + (excl + b0 > target ? 0 : excl + b0 + b1 > target ? 1 : excl + b0 + b1 + b2 > target ? 2 : 3);
        const unsigned long long hit = __ballot(med >= 0);
        if (total == 0) { if (lane == 0) s_th = -1.f; }
        else if (hit == 0) { if (lane == 0) s_th = 1.5f * 1.4f * (below256 + hist[256] > target ? 256.f : th_high); }   // the crossing is in bin 256 or 257
        else if (med >= 0) s_th = 1.5f * 1.4f * (float)med;                          // exactly one lane
    }
    __syncthreads();
    const float th = s_th;
    if (th < 0.f) return;
#pragma unroll
    for (int k = 0; k < DPT; k++) {
        const int i = threadIdx.x + 256 * k, d = dreg[k];
        if (d >= 0 && (d == SM_DIST_TH_HIGH ? !(th_high < th) : !((float)d < th))) { uRight[o + i] = -1.f; depth[o + i] = -1.f; }      // :146-155
    }
    for (int i = threadIdx.x + 256 * DPT; i < nL; i += 256) {
        int d = best_dist[o + i];
        if (d >= 0 && (d == SM_DIST_TH_HIGH ? !(th_high < th) : !((float)d < th))) { uRight[o + i] = -1.f; depth[o + i] = -1.f; }      // :146-155
    }
}

// Which instance a launch runs (hs_stereo.h).  By batch, from the sweep over 1 .. 64 pairs per call in profiles/README.md: one left keypoint per
// wave while the launch has too few workgroups to fill the chip (single pairs: the latency path, unchanged), the compacting instance with four
// keypoints per wave from 6 x 2048 slots (level with <1> at 4 pairs of 2032 slots, a fifth faster at 8), with eight from 24 x 2048 (slower than
// four at 16 pairs, faster at 32).  k_stereo_match<2>, which used to run from 8 x 2048 slots, loses to them at every size: HS_STEREO_KPW=2 only.
#define HS_STEREO_COMPACT4_MIN_SLOTS ((size_t)6 * 2048)
#define HS_STEREO_COMPACT8_MIN_SLOTS ((size_t)24 * 2048)
int hs_stereo_kpw(int knob, int pairs, int cap)
{
    if (knob == 1 || knob == 2 || knob == 4 || knob == 8) return knob;
    const size_t slots = (size_t)pairs * cap;
    return slots >= HS_STEREO_COMPACT8_MIN_SLOTS ? 8 : slots >= HS_STEREO_COMPACT4_MIN_SLOTS ? 4 : 1;
}

namespace {
void launch_match(int kpw, const int32_t* strip_count, const HsStripEntry* sl, int n_strips, const hs_keypoint* kpsL, const uint8_t* descL, const int32_t* nL,
                  const hs_keypoint* kpsR, const uint8_t* descR, const int32_t* nR, int pairs, int cap, hs_stereo_params sp, float* uRight, float* depth,
                  int32_t* best_dist, hipStream_t s)
{
    const dim3 grid((cap + 4 * kpw - 1) / (4 * kpw), pairs, 1);      // four waves per workgroup, kpw left keypoints per wave
#define SM_LAUNCH(KERNEL) hipLaunchKernelGGL(KERNEL, grid, dim3(256), 0, s, strip_count, sl, n_strips, kpsL, descL, nL, kpsR, descR, nR, cap, sp, uRight, depth, best_dist)
    if (kpw == 8) SM_LAUNCH(k_stereo_match_compact<8>);
    else if (kpw == 4) SM_LAUNCH(k_stereo_match_compact<4>);
    else if (kpw == 2) SM_LAUNCH(k_stereo_match<2>);
    else SM_LAUNCH(k_stereo_match<1>);
#undef SM_LAUNCH
}
} // namespace

void hs_launch_stereo_kpw(const hs_keypoint* kpsL, const uint8_t* descL, const int32_t* nL,
                          const hs_keypoint* kpsR, const uint8_t* descR, const int32_t* nR,
                          int pairs, int cap, hs_stereo_params sp, float* uRight, float* depth, int32_t* best_dist,
                          int32_t* strip_count, void* strip_list, int kpw_knob, hipStream_t s)
{
    if (pairs <= 0 || cap <= 0) return;
    HsStripEntry* const sl = reinterpret_cast<HsStripEntry*>(strip_list);
    const int n_strips = hs_stereo_strips(sp.n_rows);
    hipLaunchKernelGGL(k_stereo_strips, dim3(pairs), dim3(STRIPS_T), 0, s, kpsR, nR, cap, sp.size_ref, sp.n_rows, n_strips, strip_count, sl);
    launch_match(hs_stereo_kpw(kpw_knob, pairs, cap), strip_count, sl, n_strips, kpsL, descL, nL, kpsR, descR, nR, pairs, cap, sp, uRight, depth, best_dist, s);
}
void hs_launch_stereo(const hs_keypoint* kpsL, const uint8_t* descL, const int32_t* nL,
                      const hs_keypoint* kpsR, const uint8_t* descR, const int32_t* nR,
                      int pairs, int cap, hs_stereo_params sp, float* uRight, float* depth, int32_t* best_dist,
                      int32_t* strip_count, void* strip_list, hipStream_t s)
{
    hs_launch_stereo_kpw(kpsL, descL, nL, kpsR, descR, nR, pairs, cap, sp, uRight, depth, best_dist, strip_count, strip_list, 0, s);
}

void hs_launch_stereo_median(const int32_t* nL, int pairs, int cap, float* uRight, float* depth, const int32_t* best_dist, float th_high,
                             int32_t* strip_count, int n_rows, hipStream_t s)
{
    if (pairs <= 0 || cap <= 0) return;
    hipLaunchKernelGGL(k_stereo_median, dim3(pairs), dim3(256), 0, s, nL, cap, uRight, depth, best_dist, th_high, strip_count, hs_stereo_strips(n_rows));
}

// the matcher alone, on strips that the describe launch of the stereo front end has already binned (HsStripFuse)
void hs_launch_stereo_match_only_kpw(const hs_keypoint* kpsL, const uint8_t* descL, const int32_t* nL,
                                     const hs_keypoint* kpsR, const uint8_t* descR, const int32_t* nR,
                                     int pairs, int cap, hs_stereo_params sp, float* uRight, float* depth, int32_t* best_dist,
                                     const int32_t* strip_count, const void* strip_list, int kpw_knob, hipStream_t s)
{
    if (pairs <= 0 || cap <= 0) return;
    launch_match(hs_stereo_kpw(kpw_knob, pairs, cap), strip_count, reinterpret_cast<const HsStripEntry*>(strip_list), hs_stereo_strips(sp.n_rows), kpsL, descL, nL,
                 kpsR, descR, nR, pairs, cap, sp, uRight, depth, best_dist, s);
}
void hs_launch_stereo_match_only(const hs_keypoint* kpsL, const uint8_t* descL, const int32_t* nL,
                                 const hs_keypoint* kpsR, const uint8_t* descR, const int32_t* nR,
                                 int pairs, int cap, hs_stereo_params sp, float* uRight, float* depth, int32_t* best_dist,
                                 const int32_t* strip_count, const void* strip_list, hipStream_t s)
{
    hs_launch_stereo_match_only_kpw(kpsL, descL, nL, kpsR, descR, nR, pairs, cap, sp, uRight, depth, best_dist, strip_count, strip_list, 0, s);
}
