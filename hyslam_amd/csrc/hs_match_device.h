// hs_match_device.h — the device idioms shared by kernels_match.hip, kernels_bow.hip, kernels_place.hip, kernels_landmark.hip, hs_kfgraph.hip, kernels_localmap.hip and kernels_track_refkf.hip (only these include
// it).  Each helper states ONE reference rule once: first minimum wins, the (best key, second-best distance) pair, the cell range of
// GetFeaturesInArea (D7), the no-candidate second distance (D10), the rotation histogram.  Everything is force-inlined.
#pragma once
#include "hs_internal.h"
#include <cfloat>

#define GRID_COLS 64   // FRAME_GRID_COLS, src/core/Frame.h
#define GRID_ROWS 48

// ---- 256-bit descriptors
struct Desc256 { unsigned long long w[4]; };
__device__ __forceinline__ Desc256 desc_load(const uint8_t* d32)
{
    const unsigned long long* p = reinterpret_cast<const unsigned long long*>(d32);
    return Desc256{{p[0], p[1], p[2], p[3]}};
}
__device__ __forceinline__ int hamming256(const Desc256& a, const Desc256& b)
{
    return __popcll(a.w[0] ^ b.w[0]) + __popcll(a.w[1] ^ b.w[1]) + __popcll(a.w[2] ^ b.w[2]) + __popcll(a.w[3] ^ b.w[3]);
}

// ---- a value of lane j (j uniform)
__device__ __forceinline__ float lane_read(float x, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j)); }
__device__ __forceinline__ unsigned long long lane_read(unsigned long long x, int j)
{
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)x, j), hi = __builtin_amdgcn_readlane((unsigned)(x >> 32), j);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ double lane_read(double x, int j) { return __longlong_as_double((long long)lane_read((unsigned long long)__double_as_longlong(x), j)); }

// ---- (best key, second-best distance): a key is dist << 32 | tie order, so the smallest key is the reference's first minimum; the second-best
// distance is the second smallest of the multiset and does not depend on the order
#define HS_NO_KEY 0x7FFFFFFFFFFFFFFFull
#define HS_NO_DIST 0x7FFFFFFF
// one candidate
__device__ __forceinline__ void best2_take(unsigned long long& best, int& second, unsigned long long key, int d)
{
    if (key < best) { second = min(second, (int)(best >> 32)); best = key; }
    else second = min(second, d);
}
// another (best, second) pair; the distance of whichever best loses is a second-best candidate (0x7FFFFFFF when a side is empty)
__device__ __forceinline__ void best2_merge(unsigned long long& best, int& second, unsigned long long ob, int os)
{
    const int worse = max((int)(best >> 32), (int)(ob >> 32));
    best = min(best, ob);
    second = min(min(second, os), worse);
}
// the whole wave; every lane holds the result
__device__ __forceinline__ void wave_best2(unsigned long long& best, int& second)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) best2_merge(best, second, __shfl_xor(best, s, 64), __shfl_xor(second, s, 64));
}
// bestDist2 of the accept rules: FLT_MAX when there was a single candidate (D10)
__device__ __forceinline__ float second_as_float(int second) { return second == HS_NO_DIST ? FLT_MAX : (float)second; }
// BestMatchBoWCriterion (MatchCriteria.cpp:601-635); best != HS_NO_KEY.  The projection and initialization matchers' rules differ on purpose.
__device__ __forceinline__ bool bow_accept(unsigned long long best, int second, float score_threshold, float ratio)
{
    const float bd1 = (float)(int)(best >> 32);
    return bd1 < score_threshold && bd1 < __fmul_rn(ratio, second_as_float(second));
}

// ---- the cell range of GetFeaturesInArea(u, v, r) with its early returns (Frame.cc:416-457)
// (int) of an integral float (a floor / ceil / round result) as the reference's x86-64 build converts it (cvttss2si): NaN or a value outside the
// int range gives INT_MIN.  C++ leaves that conversion undefined; a plain cast here is v_cvt_i32_f32, which clamps to INT_MAX and maps NaN to 0, so
// a huge or infinite search radius would scan the whole grid where the reference finds nothing.
__device__ __forceinline__ int cvt_i32(float v) { return (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : (int)0x80000000u; }
struct GridRange { int minCX, maxCX, minCY, maxCY; bool empty; };
__device__ __forceinline__ GridRange grid_range(float min_x, float max_x, float min_y, float max_y, float u, float v, float r)
{
    const float invW = (float)GRID_COLS / (max_x - min_x), invH = (float)GRID_ROWS / (max_y - min_y);
    GridRange g;
    g.minCX = max(0, cvt_i32(floorf(__fmul_rn(__fsub_rn(__fsub_rn(u, min_x), r), invW))));
    g.maxCX = min(GRID_COLS - 1, cvt_i32(ceilf(__fmul_rn(__fadd_rn(__fsub_rn(u, min_x), r), invW))));
    g.minCY = max(0, cvt_i32(floorf(__fmul_rn(__fsub_rn(__fsub_rn(v, min_y), r), invH))));
    g.maxCY = min(GRID_ROWS - 1, cvt_i32(ceilf(__fmul_rn(__fadd_rn(__fsub_rn(v, min_y), r), invH))));
    g.empty = g.minCX >= GRID_COLS || g.maxCX < 0 || g.minCY >= GRID_ROWS || g.maxCY < 0;
    return g;
}

// ---- RotationConsistency (MatchCriteria.cpp:684-767): the 30-bin histogram of angle_a - angle_b and its three maxima
__device__ __forceinline__ int rot_bin(float angle_a, float angle_b)
{
    float rot = __fsub_rn(angle_a, angle_b);
    if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
    const int b = (int)roundf(__fmul_rn(rot, 1.0f / 30));
    return b == 30 ? 0 : b;
}
__device__ __forceinline__ void three_maxima(const int* hist, int* ind)     // ComputeThreeMaxima; one thread
{
    int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
    for (int i = 0; i < 30; i++) {
        const int s = hist[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
        else if (s > max3) { max3 = s; i3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { i3 = -1; }
    ind[0] = i1; ind[1] = i2; ind[2] = i3;
}

// ---- exclusive prefix of one value per thread over a 1024-thread workgroup (all threads call it; s_wave is the caller's LDS)
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* s_wave /*[16]*/, uint32_t& total)
{
    const int tid = threadIdx.x;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t x = __shfl_up(incl, o, 64); if ((tid & 63) >= o) incl += x; }
    if ((tid & 63) == 63) s_wave[tid >> 6] = incl;
    __syncthreads();
    uint32_t base = 0; total = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) { const uint32_t x = s_wave[w]; if (w < (tid >> 6)) base += x; total += x; }
    return base + incl - v;
}
