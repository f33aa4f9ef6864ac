// kernels_place.hip — place recognition: HYSLAM::PlaceRecognizer (src/core/PlaceRecognizer.cpp:43-311) behind KeyFrameDB::DetectRelocalizationCandidates
// / DetectLoopCandidates (KeyFrameDB.cc:392-419), on top of DBoW2's L1 score (FeatureVocabulary::score, ORBVocabulary.cpp:44-46).
//
//   hs_place_db_*            the key frames' BoW vectors resident in HBM: a CSR of (int32 word, double value) per slot, tombstones on erase
//   hs_place_query_reloc     detectRelocalizationCandidates (:201-311)
//   hs_place_query_loop      detectLoopCandidates (:81-199)
//
// The reference walks an inverted file (one std::list<KeyFrame*> per word) to count shared words and then scores the survivors one std::map merge at a
// time.  Here the inverted file does not exist: the query vector is scattered into a dense table of n_words doubles (0.0 = word absent; a stored value is
// > 0), one wavefront per stored key frame looks every word of its list up in that table, and shared-word count and L1 score come out of the same pass.
// The table is cleared again by un-scattering the query, so a query touches qm entries of it, not n_words.
//
//   k_place_scatter   query -> dense table (set) / dense table -> 0 (clear); the set pass also resets the maximum shared-word count
//   k_place_score     per slot: the reference's count (-1: not an entry), float si = (float)score for every slot that shares a word, max count
//   k_place_select    ONE workgroup: minCommonWords, the covisibility accumulation, the 0.75 retain test and the ordered, de-duplicated output
//
// Arithmetic: L1Scoring::score adds `fabs(vi - wi) - fabs(vi) - fabs(wi)` per shared word in ascending word order in double, from 0.0, and returns
// -s / 2.0; compiled with -ffp-contract=off and written with __dsub_rn / __dadd_rn so that nothing fuses.  The sum is ordered: the hits of a 64-entry
// chunk are COMPACTED (a ballot, then one readlane per hit in lane order = word order), so lanes without a hit add nothing at all.
#include "hs_match_device.h"
#include <algorithm>
#include <cmath>
#include <climits>
#include <cstring>
#include <vector>

#define PL_NEIGH 10                 // GetBestCovisibilityKeyFrames(10), PlaceRecognizer.cpp:153,267
#define PL_MAX_SLOTS (1 << 20)
#define PL_NONE 0x7FFFFFFF

__global__ __launch_bounds__(256) void k_place_scatter(const int32_t* __restrict__ qw, const double* __restrict__ qv, const int32_t* __restrict__ d_qm, int qm_max, int n_words,
                                                       double* __restrict__ dense, int32_t* __restrict__ max_count, int set)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int qm = d_qm ? min(max(*d_qm, 0), qm_max) : qm_max;
    if (i == 0 && set) *max_count = 0;
    if (i >= qm) return;
    const int w = qw[i];
    if ((unsigned)w < (unsigned)n_words) dense[w] = set ? qv[i] : 0.0;
}

// one wavefront per slot
__global__ __launch_bounds__(256) void k_place_score(const int32_t* __restrict__ pw, const double* __restrict__ pv, const int64_t* __restrict__ start, const int32_t* __restrict__ len,
                                                     int slots, int n_words, const double* __restrict__ dense, const uint8_t* __restrict__ exclude, int loop,
                                                     int32_t* __restrict__ cnt, float* __restrict__ si, int32_t* __restrict__ max_count)
{
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (slot >= slots) return;
    const int n = __builtin_amdgcn_readfirstlane(len[slot]);
    // a tombstone; or, in the loop query, a connected key frame: never in shared_words (:97)
    if (n < 0 || (exclude && __builtin_amdgcn_readfirstlane((int)exclude[slot]))) { if (lane == 0) { cnt[slot] = -1; si[slot] = 0.0f; } return; }
    const int64_t o = start[slot];
    double s = 0.0;
    int shared = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        double term = 0.0;
        bool hit = false;
        if (i < n) {
            const int w = pw[o + i];
            if ((unsigned)w < (unsigned)n_words) {
                const double vi = dense[w], wi = pv[o + i];                   // v1 = the query, v2 = the key frame (:135,251)
                if (vi > 0.0) { hit = true; term = __dsub_rn(__dsub_rn(fabs(__dsub_rn(vi, wi)), fabs(vi)), fabs(wi)); }
            }
        }
        unsigned long long m = __ballot(hit);
        shared += __popcll(m);
        while (m) {                                                             // the chunk's hits, in lane order = ascending word order
            const int j = __builtin_ctzll(m);
            m &= m - 1;
            s = __dadd_rn(s, lane_read(term, j));
        }
    }
    if (lane != 0) return;
    // reloc: mnRelocWords (:218-222).  loop: shared_words starts an entry at 0 and counts from the SECOND hit (:98-102)
    const int c = shared > 0 ? shared - (loop ? 1 : 0) : -1;
    cnt[slot] = c;
    si[slot] = shared > 0 ? __double2float_rn(__ddiv_rn(-s, 2.0)) : 0.0f;      // float si = mpVoc->score(...)
    if (c > 0) atomicMax(max_count, c);
}

struct PlSelArgs {
    int slots, n_live, loop, cap;
    float min_score;
    const int32_t* order;            // live slots in ascending key order
    const int32_t* neigh;            // [slots][PL_NEIGH] or nullptr
    const int32_t* cnt; const float* si; const int32_t* max_count;
    int32_t* first; float* acc; int32_t* best; int32_t* cand; int32_t* n_cand;
};

__device__ __forceinline__ int pl_block_sum(int v, int* s_w)     // all 1024 threads; result in every thread
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) t += s_w[w];
    return t;
}

__global__ __launch_bounds__(1024) void k_place_select(PlSelArgs a)
{
    __shared__ int s_w[16];
    __shared__ float s_f[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < a.slots; i += 1024) { a.first[i] = PL_NONE; a.acc[i] = 0.0f; a.best[i] = -1; }
    __syncthreads();
    const int max_common = *a.max_count;
    const int min_common = (int)__fmul_rn((float)max_common, 0.8f);             // int minCommonWords = maxCommonWords*0.8f (:121,237)
    float best_acc = a.loop ? a.min_score : 0.0f;                               // bestAccScore (:147,261)
    for (int e = tid; e < a.n_live; e += 1024) {
        const int slot = a.order[e];
        if (!(a.cnt[slot] > min_common)) continue;                              // (:131,248); -1 never passes
        const float s0 = a.si[slot];
        if (a.loop && !(s0 >= a.min_score)) continue;                           // (:138)
        float best_score = s0, acc = s0;
        int best = slot;
        if (a.neigh)
            for (int k = 0; k < PL_NEIGH; k++) {
                const int nb = a.neigh[(size_t)slot * PL_NEIGH + k];
                if (nb < 0 || nb >= a.slots) continue;
                const int c = a.cnt[nb];
                // reloc: mnRelocQuery == F->mnId, i.e. shares a word (:275; its score by DESIGN.md D9).  loop: an entry above minCommonWords (:161-162)
                if (a.loop ? !(c > min_common) : c < 0) continue;
                const float s2 = a.si[nb];
                acc = __fadd_rn(acc, s2);
                if (s2 > best_score) { best = nb; best_score = s2; }
            }
        a.acc[slot] = acc; a.best[slot] = best;
        if (acc > best_acc) best_acc = acc;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best_acc = fmaxf(best_acc, __shfl_xor(best_acc, o, 64));
    if (lane == 0) s_f[wv] = best_acc;
    __syncthreads();                                                            // also: acc / best of every slot are visible
#pragma unroll
    for (int w = 0; w < 16; w++) best_acc = fmaxf(best_acc, s_f[w]);
    const float retain = __fmul_rn(0.75f, best_acc);                            // minScoreToRetain (:178,292)
    for (int e = tid; e < a.n_live; e += 1024) {
        const int slot = a.order[e], b = a.best[slot];
        if (b < 0 || !(a.acc[slot] > retain)) continue;                         // (:186,299)
        if (a.loop) atomicMin(&a.first[b], e);                                  // the first entry of the walk that names b
        else a.first[b] = 0;                                                    // member of the result set
    }
    __syncthreads();
    // loop: pBestKF of every retained entry in walk order, first occurrence only.  reloc: the set's members in ascending key order.
    auto emits = [&](int e, int& out) {
        if (e >= a.n_live) return false;
        const int slot = a.order[e];
        if (!a.loop) { out = slot; return a.first[slot] == 0; }
        const int b = a.best[slot];
        out = b;
        return b >= 0 && a.acc[slot] > retain && a.first[b] == e;
    };
    int mine = 0, dummy;
    for (int e = tid; e < a.n_live; e += 1024) mine += emits(e, dummy) ? 1 : 0;
    const int total = pl_block_sum(mine, s_w);
    if (tid == 0) *a.n_cand = total;
    if (total == 0 || total > a.cap) return;                                    // too small a `cap`: the count only, no candidate
    int base = 0;
    for (int e0 = 0; e0 < a.n_live; e0 += 1024) {
        int out = -1;
        const bool p = emits(e0 + tid, out);
        const unsigned long long m = __ballot(p);
        const int within = __popcll(m & ((1ull << lane) - 1ull));
        __syncthreads();
        if (lane == 0) s_w[wv] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) { const int x = s_w[w]; if (w < wv) before += x; all += x; }
        if (p) a.cand[base + before + within] = out;
        base += all;
    }
}

struct hs_place_db {
    hs_orb* h = nullptr;
    int device = 0, n_words = 0;
    // host mirror of the slots
    std::vector<uint64_t> key; std::vector<uint8_t> live;
    std::vector<int32_t> order; bool order_dirty = true; int n_live = 0;
    int64_t pool_used = 0, pool_cap = 0;
    int slot_cap = 0;
    // device: the CSR ...
    int32_t* d_pw = nullptr; double* d_pv = nullptr; int64_t* d_start = nullptr; int32_t* d_len = nullptr;   // len -1: tombstone
    // ... the key order, the dense query table, per-slot results of the last query (also the outputs a caller did not ask for)
    int32_t* d_order = nullptr; double* d_dense = nullptr; int32_t* d_state = nullptr;                         // state[0] max count, [1] n_cand of the host forms
    int32_t* d_cnt = nullptr; float* d_si = nullptr; float* d_acc = nullptr; int32_t* d_best = nullptr; int32_t* d_first = nullptr;
    // ... staging of the host-pointer forms
    int32_t* d_neigh = nullptr; uint8_t* d_excl = nullptr; int32_t* d_cand = nullptr;
    int32_t* d_qw = nullptr; double* d_qv = nullptr; int q_cap = 0;
};

namespace {
int pl_fail(hs_place_db* db, int code, const char* msg) { hs_set_error(db->h, msg); return code; }
#define PL_TRY(db, expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { (void)hipGetLastError(); return pl_fail(db, HS_ERR_HIP, hipGetErrorString(e__)); } } while (0)

template <typename T> hipError_t pl_regrow(T*& p, size_t old_n, size_t new_n, bool keep)
{
    T* q = nullptr;
    hipError_t e = hipMalloc(&q, std::max(new_n, (size_t)1) * sizeof(T));
    if (e == hipSuccess) e = hs_poison_fresh(q, std::max(new_n, (size_t)1) * sizeof(T));
    if (e != hipSuccess) { (void)hipFree(q); return e; }
    if (keep && p && old_n) e = hipMemcpy(q, p, old_n * sizeof(T), hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { hipFree(q); return e; }
    hipFree(p);
    p = q;
    return hipSuccess;
}

// room for one more slot of `m` entries; reallocations drain the device first (rare: capacities double)
int pl_reserve(hs_place_db* db, int64_t m)
{
    const int slots = (int)db->key.size();
    if (slots >= PL_MAX_SLOTS) return pl_fail(db, HS_ERR_CAPACITY, "place database: more than 2^20 slots (clear() reuses them)");
    if (slots + 1 > db->slot_cap) {
        const int nc = std::min(PL_MAX_SLOTS, std::max(1024, db->slot_cap * 2));
        PL_TRY(db, hipDeviceSynchronize());
        PL_TRY(db, pl_regrow(db->d_start, slots, nc, true));
        PL_TRY(db, pl_regrow(db->d_len, slots, nc, true));
        PL_TRY(db, pl_regrow(db->d_order, 0, nc, false));
        PL_TRY(db, pl_regrow(db->d_cnt, 0, nc, false));
        PL_TRY(db, pl_regrow(db->d_si, 0, nc, false));
        PL_TRY(db, pl_regrow(db->d_acc, 0, nc, false));
        PL_TRY(db, pl_regrow(db->d_best, 0, nc, false));
        PL_TRY(db, pl_regrow(db->d_first, 0, nc, false));
        PL_TRY(db, pl_regrow(db->d_neigh, 0, (size_t)nc * PL_NEIGH, false));
        PL_TRY(db, pl_regrow(db->d_excl, 0, nc, false));
        PL_TRY(db, pl_regrow(db->d_cand, 0, nc, false));
        db->slot_cap = nc;
        db->order_dirty = true;
    }
    if (db->pool_used + m > db->pool_cap) {
        const int64_t nc = std::max<int64_t>(std::max<int64_t>(1 << 16, db->pool_cap * 2), db->pool_used + m);
        PL_TRY(db, hipDeviceSynchronize());
        PL_TRY(db, pl_regrow(db->d_pw, (size_t)db->pool_used, (size_t)nc, true));
        PL_TRY(db, pl_regrow(db->d_pv, (size_t)db->pool_used, (size_t)nc, true));
        db->pool_cap = nc;
    }
    return HS_OK;
}

int pl_check_vector(hs_place_db* db, const int32_t* word, const double* value, int m)
{
    for (int i = 0; i < m; i++) {
        if (word[i] < 0 || word[i] >= db->n_words || (i > 0 && word[i] <= word[i - 1])) return pl_fail(db, HS_ERR_INVALID, "BoW vector: words must be ascending, unique and < n_words");
        if (!(value[i] > 0.0) || !std::isfinite(value[i])) return pl_fail(db, HS_ERR_INVALID, "BoW vector: values must be finite and > 0");
    }
    return HS_OK;
}

__global__ void k_place_commit(int64_t* start, int32_t* len, int slot, int64_t at, const int32_t* d_m, int m_max)
{
    start[slot] = at;
    len[slot] = d_m ? min(max(*d_m, 0), m_max) : m_max;
}

int pl_new_slot(hs_place_db* db, uint64_t key, int64_t m)
{
    const int slot = (int)db->key.size();
    db->key.push_back(key); db->live.push_back(1);
    db->pool_used += m; db->n_live++; db->order_dirty = true;
    return slot;
}

// everything in device memory, on stream s
int pl_query(hs_place_db* db, int loop, const int32_t* d_qw, const double* d_qv, const int32_t* d_qm, int qm_max, const uint8_t* d_excl, float min_score,
             const int32_t* d_neigh, int32_t* d_cand, int cap, int32_t* d_ncand, int32_t* d_words, float* d_score, float* d_acc, int32_t* d_best, hipStream_t s)
{
    const int slots = (int)db->key.size();
    if (slots == 0) { PL_TRY(db, hipMemsetAsync(d_ncand, 0, 4, s)); return HS_OK; }      // nothing per slot to write either; all tombstones: the passes run (-1 / 0 everywhere)
    if (db->order_dirty) {                                                       // first query after add / erase / clear: the walk order by key
        db->order.clear();
        for (int i = 0; i < slots; i++) if (db->live[i]) db->order.push_back(i);
        std::sort(db->order.begin(), db->order.end(), [db](int x, int y) { return db->key[x] < db->key[y]; });
        PL_TRY(db, hipStreamSynchronize(s));
        if (!db->order.empty()) PL_TRY(db, hipMemcpy(db->d_order, db->order.data(), db->order.size() * 4, hipMemcpyHostToDevice));
        db->order_dirty = false;
    }
    int32_t* cnt = d_words ? d_words : db->d_cnt; float* si = d_score ? d_score : db->d_si;
    float* acc = d_acc ? d_acc : db->d_acc; int32_t* best = d_best ? d_best : db->d_best;
    const int qgrid = std::max(1, (qm_max + 255) / 256);
    hipLaunchKernelGGL(k_place_scatter, dim3(qgrid), dim3(256), 0, s, d_qw, d_qv, d_qm, qm_max, db->n_words, db->d_dense, db->d_state, 1);
    hipLaunchKernelGGL(k_place_score, dim3((slots + 3) / 4), dim3(256), 0, s, db->d_pw, db->d_pv, db->d_start, db->d_len, slots, db->n_words, db->d_dense,
                       loop ? d_excl : nullptr, loop, cnt, si, db->d_state);
    hipLaunchKernelGGL(k_place_scatter, dim3(qgrid), dim3(256), 0, s, d_qw, d_qv, d_qm, qm_max, db->n_words, db->d_dense, db->d_state, 0);
    const PlSelArgs a{slots, db->n_live, loop, cap, min_score, db->d_order, d_neigh, cnt, si, db->d_state, db->d_first, acc, best, d_cand, d_ncand};
    hipLaunchKernelGGL(k_place_select, dim3(1), dim3(1024), 0, s, a);
    PL_TRY(db, hipGetLastError());
    return HS_OK;
}

int pl_query_host(hs_place_db* db, int loop, const int32_t* qword, const double* qvalue, int qm, const uint8_t* exclude, float min_score, const int32_t* neigh,
                  int32_t* cand_slot, int cap, int32_t* n_cand, int32_t* words, float* score, float* acc, int32_t* best)
{
    if (!db) return HS_ERR_INVALID;
    if (qm < 0 || (qm > 0 && (!qword || !qvalue)) || cap < 0 || (cap > 0 && !cand_slot) || !n_cand) return pl_fail(db, HS_ERR_INVALID, "bad argument");
    const int st = pl_check_vector(db, qword, qvalue, qm);
    if (st != HS_OK) return st;
    *n_cand = 0;
    const int slots = (int)db->key.size();
    if (slots == 0) return HS_OK;
    PL_TRY(db, hipSetDevice(db->device));
    const hipStream_t s = hs_orb_stream_of(db->h);
    if (qm > db->q_cap) {
        PL_TRY(db, hipStreamSynchronize(s));
        PL_TRY(db, pl_regrow(db->d_qw, 0, (size_t)qm, false));
        PL_TRY(db, pl_regrow(db->d_qv, 0, (size_t)qm, false));
        db->q_cap = qm;
    }
    if (qm) { PL_TRY(db, hipMemcpyAsync(db->d_qw, qword, (size_t)qm * 4, hipMemcpyHostToDevice, s)); PL_TRY(db, hipMemcpyAsync(db->d_qv, qvalue, (size_t)qm * 8, hipMemcpyHostToDevice, s)); }
    if (neigh) PL_TRY(db, hipMemcpyAsync(db->d_neigh, neigh, (size_t)slots * PL_NEIGH * 4, hipMemcpyHostToDevice, s));
    if (loop && exclude) PL_TRY(db, hipMemcpyAsync(db->d_excl, exclude, (size_t)slots, hipMemcpyHostToDevice, s));
    const int q = pl_query(db, loop, db->d_qw, db->d_qv, nullptr, qm, (loop && exclude) ? db->d_excl : nullptr, min_score, neigh ? db->d_neigh : nullptr,
                           db->d_cand, slots, db->d_state + 1, nullptr, nullptr, nullptr, nullptr, s);
    if (q != HS_OK) return q;
    int32_t n = 0;
    PL_TRY(db, hipMemcpyAsync(&n, db->d_state + 1, 4, hipMemcpyDeviceToHost, s));
    PL_TRY(db, hipStreamSynchronize(s));
    if (n > cap) { *n_cand = n; return pl_fail(db, HS_ERR_CAPACITY, "place query: more candidates than `cap` (n_cand holds the count)"); }
    if (n) PL_TRY(db, hipMemcpy(cand_slot, db->d_cand, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (words) PL_TRY(db, hipMemcpy(words, db->d_cnt, (size_t)slots * 4, hipMemcpyDeviceToHost));
    if (score) PL_TRY(db, hipMemcpy(score, db->d_si, (size_t)slots * 4, hipMemcpyDeviceToHost));
    if (acc) PL_TRY(db, hipMemcpy(acc, db->d_acc, (size_t)slots * 4, hipMemcpyDeviceToHost));
    if (best) PL_TRY(db, hipMemcpy(best, db->d_best, (size_t)slots * 4, hipMemcpyDeviceToHost));
    *n_cand = n;
    return HS_OK;
}
}  // namespace

extern "C" {

int hs_place_db_create(hs_orb* h, int n_words, int scoring, hs_place_db** out)
{
    if (!h || !out) return HS_ERR_INVALID;
    *out = nullptr;
    if (n_words < 1) { hs_set_error(h, "place database: n_words < 1"); return HS_ERR_INVALID; }
    if (scoring != 0) { hs_set_error(h, "place database: only L1_NORM scoring (0) is implemented, the one hySLAM's vocabulary uses"); return HS_ERR_INVALID; }
    hs_place_db* db = new hs_place_db();
    db->h = h; db->device = hs_orb_device_of(h); db->n_words = n_words;
    hipError_t e = hipSetDevice(db->device);
    if (e == hipSuccess) e = hipMalloc(&db->d_dense, (size_t)n_words * 8);
    if (e == hipSuccess) e = hs_poison_fresh(db->d_dense, (size_t)n_words * 8);
    if (e == hipSuccess) e = hipMemset(db->d_dense, 0, (size_t)n_words * 8);
    if (e == hipSuccess) e = hipMalloc(&db->d_state, 64);
    if (e == hipSuccess) e = hs_poison_fresh(db->d_state, 64);
    if (e == hipSuccess) e = hipMemset(db->d_state, 0, 64);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { (void)hipGetLastError(); hs_set_error(h, hipGetErrorString(e)); hs_place_db_destroy(db); return HS_ERR_HIP; }
    *out = db;
    return HS_OK;
}

void hs_place_db_destroy(hs_place_db* db)
{
    if (!db) return;
    (void)hipSetDevice(db->device);
    (void)hipDeviceSynchronize();
    hipFree(db->d_pw); hipFree(db->d_pv); hipFree(db->d_start); hipFree(db->d_len); hipFree(db->d_order); hipFree(db->d_dense); hipFree(db->d_state);
    hipFree(db->d_cnt); hipFree(db->d_si); hipFree(db->d_acc); hipFree(db->d_best); hipFree(db->d_first);
    hipFree(db->d_neigh); hipFree(db->d_excl); hipFree(db->d_cand); hipFree(db->d_qw); hipFree(db->d_qv);
    delete db;
}

int hs_place_db_add(hs_place_db* db, uint64_t key, const int32_t* word, const double* value, int m, int32_t* slot)
{
    if (!db) return HS_ERR_INVALID;
    if (m < 0 || (m > 0 && (!word || !value)) || !slot) return pl_fail(db, HS_ERR_INVALID, "bad argument");
    int st = pl_check_vector(db, word, value, m);
    if (st != HS_OK) return st;
    PL_TRY(db, hipSetDevice(db->device));
    if ((st = pl_reserve(db, m)) != HS_OK) return st;
    const hipStream_t s = hs_orb_stream_of(db->h);
    const int64_t at = db->pool_used;
    if (m) { PL_TRY(db, hipMemcpyAsync(db->d_pw + at, word, (size_t)m * 4, hipMemcpyHostToDevice, s)); PL_TRY(db, hipMemcpyAsync(db->d_pv + at, value, (size_t)m * 8, hipMemcpyHostToDevice, s)); }
    hipLaunchKernelGGL(k_place_commit, dim3(1), dim3(1), 0, s, db->d_start, db->d_len, (int)db->key.size(), at, (const int32_t*)nullptr, m);
    PL_TRY(db, hipGetLastError());
    PL_TRY(db, hipStreamSynchronize(s));
    *slot = pl_new_slot(db, key, m);
    return HS_OK;
}

int hs_place_db_add_device(hs_place_db* db, uint64_t key, const int32_t* d_word, const double* d_value, const int32_t* d_m, int m_max, int32_t* slot, void* stream)
{
    if (!db) return HS_ERR_INVALID;
    if (m_max < 0 || (m_max > 0 && (!d_word || !d_value)) || !slot || ((uintptr_t)d_value & 7)) return pl_fail(db, HS_ERR_INVALID, "bad argument");
    PL_TRY(db, hipSetDevice(db->device));
    const int st = pl_reserve(db, m_max);
    if (st != HS_OK) return st;
    const hipStream_t s = hs_stream_or(db->h, stream);
    const int64_t at = db->pool_used;
    if (m_max) {
        PL_TRY(db, hipMemcpyAsync(db->d_pw + at, d_word, (size_t)m_max * 4, hipMemcpyDeviceToDevice, s));
        PL_TRY(db, hipMemcpyAsync(db->d_pv + at, d_value, (size_t)m_max * 8, hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(k_place_commit, dim3(1), dim3(1), 0, s, db->d_start, db->d_len, (int)db->key.size(), at, d_m, m_max);
    PL_TRY(db, hipGetLastError());
    *slot = pl_new_slot(db, key, m_max);
    return HS_OK;
}

int hs_place_db_erase(hs_place_db* db, int32_t slot)
{
    if (!db) return HS_ERR_INVALID;
    if (slot < 0 || slot >= (int)db->key.size() || !db->live[slot]) return pl_fail(db, HS_ERR_INVALID, "place database: no live entry in this slot");
    PL_TRY(db, hipSetDevice(db->device));
    const int32_t dead = -1;
    PL_TRY(db, hipDeviceSynchronize());                                         // queries in flight still see the entry
    PL_TRY(db, hipMemcpy(db->d_len + slot, &dead, 4, hipMemcpyHostToDevice));
    db->live[slot] = 0; db->n_live--; db->order_dirty = true;
    return HS_OK;
}

int hs_place_db_clear(hs_place_db* db)
{
    if (!db) return HS_ERR_INVALID;
    PL_TRY(db, hipSetDevice(db->device));
    PL_TRY(db, hipDeviceSynchronize());
    db->key.clear(); db->live.clear(); db->order.clear();
    db->pool_used = 0; db->n_live = 0; db->order_dirty = true;
    return HS_OK;
}

int hs_place_db_size(const hs_place_db* db, int32_t* live, int32_t* slots)
{
    if (!db) return HS_ERR_INVALID;
    if (live) *live = db->n_live;
    if (slots) *slots = (int32_t)db->key.size();
    return HS_OK;
}

int hs_place_query_reloc(hs_place_db* db, const int32_t* qword, const double* qvalue, int qm, const int32_t* neigh,
                         int32_t* cand_slot, int cap, int32_t* n_cand, int32_t* words, float* score, float* acc, int32_t* best)
{
    return pl_query_host(db, 0, qword, qvalue, qm, nullptr, 0.0f, neigh, cand_slot, cap, n_cand, words, score, acc, best);
}

int hs_place_query_loop(hs_place_db* db, const int32_t* qword, const double* qvalue, int qm, const uint8_t* exclude, float min_score, const int32_t* neigh,
                        int32_t* cand_slot, int cap, int32_t* n_cand, int32_t* words, float* score, float* acc, int32_t* best)
{
    return pl_query_host(db, 1, qword, qvalue, qm, exclude, min_score, neigh, cand_slot, cap, n_cand, words, score, acc, best);
}

static int pl_query_device_checked(hs_place_db* db, int loop, const int32_t* d_qword, const double* d_qvalue, const int32_t* d_qm, int qm_max, const uint8_t* d_exclude,
                                   float min_score, const int32_t* d_neigh, int32_t* d_cand_slot, int cap, int32_t* d_n_cand,
                                   int32_t* d_words, float* d_score, float* d_acc, int32_t* d_best, void* stream)
{
    if (!db) return HS_ERR_INVALID;
    if (qm_max < 0 || (qm_max > 0 && (!d_qword || !d_qvalue)) || cap < 0 || (cap > 0 && !d_cand_slot) || !d_n_cand || ((uintptr_t)d_qvalue & 7))
        return pl_fail(db, HS_ERR_INVALID, "bad argument");
    PL_TRY(db, hipSetDevice(db->device));
    return pl_query(db, loop, d_qword, d_qvalue, d_qm, qm_max, d_exclude, min_score, d_neigh, d_cand_slot, cap, d_n_cand, d_words, d_score, d_acc, d_best,
                    hs_stream_or(db->h, stream));
}

int hs_place_query_reloc_device(hs_place_db* db, const int32_t* d_qword, const double* d_qvalue, const int32_t* d_qm, int qm_max, const int32_t* d_neigh,
                                int32_t* d_cand_slot, int cap, int32_t* d_n_cand, int32_t* d_words, float* d_score, float* d_acc, int32_t* d_best, void* stream)
{
    return pl_query_device_checked(db, 0, d_qword, d_qvalue, d_qm, qm_max, nullptr, 0.0f, d_neigh, d_cand_slot, cap, d_n_cand, d_words, d_score, d_acc, d_best, stream);
}

int hs_place_query_loop_device(hs_place_db* db, const int32_t* d_qword, const double* d_qvalue, const int32_t* d_qm, int qm_max, const uint8_t* d_exclude, float min_score,
                               const int32_t* d_neigh, int32_t* d_cand_slot, int cap, int32_t* d_n_cand, int32_t* d_words, float* d_score, float* d_acc, int32_t* d_best,
                               void* stream)
{
    return pl_query_device_checked(db, 1, d_qword, d_qvalue, d_qm, qm_max, d_exclude, min_score, d_neigh, d_cand_slot, cap, d_n_cand, d_words, d_score, d_acc, d_best, stream);
}

}  // extern "C"
