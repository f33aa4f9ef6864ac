// host_sanitize.cpp — drives the PRODUCT's host code (everything in hyslam_amd/csrc that does not run on the GPU) under AddressSanitizer +
// UndefinedBehaviorSanitizer, CPU only: the library's translation units compiled host-only and linked against hip_stub.cpp (device memory =
// host memory, launches = no-ops).  Covered: hs_orb_create's tables, configure_impl's geometry for a random sweep of frame sizes / scale factors /
// level counts / cell sizes / feature counts (the sweep of tests/test_gpu_parity.py plus extremes): pyramid fusion, chain and deep-chain planners,
// FAST work items (wide and narrow), quadtree key tables, workspace sizing and uploads; the host-pointer entry points' staging (extract, batch,
// stereo, the matchers' CSR / scratch handling, and a sweep of all thirteen entry points that stage through HsStage on ONE handle, so that its scratch
// arena grows and is reused: staged_sweep), the ingest ticket state machine (submit / wait, errors, both slots busy), and the vocabulary
// loaders on valid, truncated and randomly corrupted text / binary files (hs_vocab_last_error instead of stderr); the host-pointer forms of the key-frame
// graph, the local map and the pose optimiser, the *_work_bytes functions and the `_device` forms of the tracking, reference-key-frame and key-frame
// stages on work areas of exactly the stated size (map_sweep); the place database's slot mirror, tombstones, both regrow paths and the key-order
// upload (place_section).  The same file builds under ThreadSanitizer (make SAN=thread): `threads <seed>` runs the sections that share something
// between threads — handle destruction against the last borrower, the frame cache, the sweeps on four threads with handles of their own, handle
// churn beside extraction and matching, place databases with and without a mutex, the vocabulary loaders and hs_comm_available's first call.
// usage: host_sanitize [seed] [geometries] [vocab_cases]      prints "HOST SANITIZE OK ..." (any sanitizer report aborts with a non-zero status)
//        host_sanitize threads [seed]                         prints "HOST SANITIZE THREADS OK ..."
//        host_sanitize plan W H [nfeat scale levels [cell]]   the host-side plan of a geometry
//        host_sanitize refusals [list]                        prints "HOST SANITIZE REFUSALS OK ..." (list: every call's status first)
//        host_sanitize fastplan                               the FAST launch plan under the environment's knobs: one digest line per tile width, one for the narrow / wide choice
//        host_sanitize fastsched                              the FAST work-unit schedule, host half and device half together; prints "FAST SCHEDULE OK ..."
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <vector>
#include <thread>
#include <atomic>
#include <mutex>
#include <cmath>
#include <limits>
#include <unistd.h>
#include "../../../include/hyslam_amd.h"
#include "../../../hyslam_amd/csrc/hs_plan.h"   // the FAST launch plan and schedule (hs_fast.h) and the knob table's reader: pure host code, called directly
void hs_orb_borrow(hs_orb* h, int delta);      // hs_api.hip (internal: what hs_comm_create / hs_comm_destroy call)

extern "C" long hip_stub_launches();
extern "C" void hip_stub_zero_device();
extern "C" void hip_stub_counters(unsigned long long* out /*[14]*/);       // hip_stub.cpp: live allocations, calls and bytes of allocations / copies / memsets, launches and their digest
uint64_t hs_debug_plan_digest(const hs_orb* h);                           // hs_api.hip: FNV-style 64-bit digest of the pointer-free plan of the current configuration (hs_plan.h)
void hs_debug_plan_summary(const hs_orb* h, int32_t* out /*[8]*/);        // hs_api.hip: launches of the pyramid's two plans, item counts (host-side facts of the last configuration)

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static thread_local std::mt19937_64 rng;      // one per thread: the main thread's is what the seed made it, whatever the other threads draw
static int rnd(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }

// what the host code asked of the runtime so far, as one line: two commits that claim the same behaviour print the same figures
static void print_counters(const char* where)
{
    unsigned long long c[14]; hip_stub_counters(c);
    printf("%s: live device %llu pinned %llu | hipMalloc %llu calls %llu B | hipHostMalloc %llu calls %llu B | H2D %llu calls %llu B | D2H %llu calls %llu B | memset %llu calls %llu B | launches %llu digest %016llx\n",
           where, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], c[10], c[11], c[12], c[13]);
}
// live "device" and pinned allocations: a handle that was destroyed must have given back everything it took
struct Live { unsigned long long dev, pin; };
static Live live_now() { unsigned long long c[14]; hip_stub_counters(c); return Live{ c[0], c[1] }; }
static bool same_live(const Live& a) { const Live b = live_now(); if (a.dev != b.dev || a.pin != b.pin) printf("live allocations: device %llu -> %llu, pinned %llu -> %llu\n", a.dev, b.dev, a.pin, b.pin); return a.dev == b.dev && a.pin == b.pin; }

static int geometry_case(int w, int h, int nfeat, float scale, int levels, int cell, int batch, bool exercise)
{
    hs_orb_params p; hs_orb_default_params(&p);
    p.nfeatures = nfeat; p.scale_factor = scale; p.nlevels = levels; p.cell_px = cell;
    hs_orb* ex = nullptr;
    const Live before = live_now();
    int st = hs_orb_create(&p, 0, &ex);
    if (st != HS_OK) return 0;                                   // rejected parameter combinations (quota > LDS list, ...) are fine: no crash is the point
    st = hs_orb_reserve(ex, w, h, batch);
    int ok = 0;
    if (st != HS_OK && std::strstr(hs_orb_last_error(ex), "internal:")) { printf("reserve %dx%d: %s\n", w, h, hs_orb_last_error(ex)); return -1; }   // a refusal is fine, a failed self-check is not
    if (st == HS_OK) {
        ok = 1;
        int32_t plan[8]; hs_debug_plan_summary(ex, plan);
        if (plan[0] <= 0 && levels > 1) { printf("no pyramid launches for %dx%d levels %d\n", w, h, levels); return -1; }
        const int cap = hs_orb_max_keypoints(ex);
        if (exercise && cap > 0) {
            std::vector<uint8_t> img((size_t)w * h);
            for (auto& v : img) v = (uint8_t)rng();
            std::vector<hs_keypoint> k((size_t)batch * cap); std::vector<uint8_t> d((size_t)batch * cap * 32); std::vector<int32_t> n(batch, -1);
            std::vector<const uint8_t*> ptrs(batch, img.data());
            st = hs_orb_extract_batch(ex, ptrs.data(), batch, w, h, w, k.data(), d.data(), cap, n.data());
            if (st != HS_OK) { printf("extract_batch %dx%d: %s\n", w, h, hs_orb_last_error(ex)); return -1; }
            {   // the camera-frame entry point (PreProcessImg on the device): a 3-channel frame of TWICE the size at scale 0.5 lands on the same level-0 geometry,
                // a 4-channel frame at scale 1 too; the staging of the raw frames (row padding to 4 bytes, odd strides) and the grey read-back run under the sanitizers
                hs_preprocess_params pp{ 3, 1, 0.5f, 0 };
                int32_t ow = 0, oh = 0; hs_preprocess_size(2 * w, 2 * h, pp.scale, &ow, &oh);
                if (ow != w || oh != h) { printf("hs_preprocess_size(%d, %d, 0.5) = %d x %d\n", 2 * w, 2 * h, ow, oh); return -1; }
                std::vector<uint8_t> col((size_t)2 * w * 3 * 2 * h + 16), grey((size_t)batch * w * h);
                for (auto& v : col) v = (uint8_t)rng();
                std::vector<const uint8_t*> cptrs(batch, col.data());
                st = hs_orb_extract_camera_batch(ex, cptrs.data(), batch, 2 * w, 2 * h, (size_t)2 * w * 3, &pp, k.data(), d.data(), cap, n.data(), grey.data());
                if (st != HS_OK) { printf("extract_camera_batch %dx%d: %s\n", w, h, hs_orb_last_error(ex)); return -1; }
                hs_preprocess_params p4{ 4, 0, 1.0f, 0 };
                std::vector<uint8_t> c4((size_t)(w * 4 + 3) * h);
                std::vector<const uint8_t*> c4p(batch, c4.data());
                st = hs_orb_extract_camera_batch(ex, c4p.data(), batch, w, h, (size_t)w * 4 + 3, &p4, k.data(), d.data(), cap, n.data(), nullptr);
                if (st != HS_OK) { printf("extract_camera_batch (4 channels) %dx%d: %s\n", w, h, hs_orb_last_error(ex)); return -1; }
                hs_preprocess_params bad{ 2, 0, 1.0f, 0 };
                if (hs_orb_extract_camera_batch(ex, c4p.data(), batch, w, h, (size_t)w * 4 + 3, &bad, k.data(), d.data(), cap, n.data(), nullptr) == HS_OK) { printf("two channels were accepted\n"); return -1; }
            }
            // the ingest tickets: two in flight, a third is refused, waits in both orders, a wait with too small a capacity keeps the ticket
            hs_stereo_params sp{ 500.f, 60.f, h, 100.f, 50.f, 31.f };
            if (batch % 2 == 0) {
                int32_t t1 = 0, t2 = 0, t3 = 0;
                if (hs_orb_submit_batch(ex, ptrs.data(), batch, w, h, w, &sp, &t1) != HS_OK) { printf("submit: %s\n", hs_orb_last_error(ex)); return -1; }
                if (hs_orb_submit_batch(ex, ptrs.data(), batch, w, h, w, &sp, &t2) != HS_OK) return -1;
                if (hs_orb_submit_batch(ex, ptrs.data(), batch, w, h, w, &sp, &t3) == HS_OK) { printf("a third ticket was accepted\n"); return -1; }
                std::vector<float> ur((size_t)batch / 2 * cap), dz((size_t)batch / 2 * cap);
                if (hs_orb_wait(ex, t2, k.data(), d.data(), n.data(), 1, ur.data(), dz.data()) == HS_OK) { printf("a wait with cap 1 passed\n"); return -1; }      // (the ticket stays valid)
                if (hs_orb_wait(ex, t2, k.data(), d.data(), n.data(), cap, ur.data(), dz.data()) != HS_OK) { printf("wait t2: %s\n", hs_orb_last_error(ex)); return -1; }
                if (hs_orb_wait(ex, t1, k.data(), d.data(), n.data(), cap, ur.data(), dz.data()) != HS_OK) return -1;
                if (hs_orb_wait(ex, t1, k.data(), d.data(), n.data(), cap, ur.data(), dz.data()) == HS_OK) { printf("a ticket was waited for twice\n"); return -1; }
            }
            // stereo matcher + 2-NN on host arrays (staging sizes follow nL / nR)
            const int nL = rnd(0, 300), nR = rnd(0, 300);
            std::vector<hs_keypoint> kl(std::max(nL, 1)), kr(std::max(nR, 1)); std::vector<uint8_t> dl((size_t)std::max(nL, 1) * 32), dr((size_t)std::max(nR, 1) * 32);
            for (auto& q : kl) { q.x = (float)rnd(0, w); q.y = (float)rnd(-5, h + 5); q.size = 31.f; q.octave = rnd(0, 7); }
            for (auto& q : kr) { q.x = (float)rnd(0, w); q.y = (float)rnd(-5, h + 5); q.size = 31.f; q.octave = rnd(0, 7); }
            std::vector<float> ur(std::max(nL, 1)), dz(std::max(nL, 1));
            if (hs_stereo_match(ex, kl.data(), dl.data(), nL, kr.data(), dr.data(), nR, &sp, ur.data(), dz.data()) != HS_OK) { printf("stereo: %s\n", hs_orb_last_error(ex)); return -1; }
            std::vector<int32_t> bi(std::max(nL, 1)), bd(std::max(nL, 1)), sd(std::max(nL, 1));
            if (nL > 0 && nR > 0 && hs_hamming_knn2(ex, dl.data(), nL, dr.data(), nR, bi.data(), bd.data(), sd.data()) != HS_OK) return -1;
        }
    }
    hs_orb_destroy(ex);
    if (!same_live(before)) { printf("hs_orb_destroy left allocations behind (%dx%d, batch %d)\n", w, h, batch); return -1; }
    return ok;
}

// a small valid vocabulary (k-ary tree of `levels` levels), saved as text and binary through the library's own writer
static hs_vocab* make_vocab(int k, int levels, std::vector<int32_t>& cb, std::vector<int32_t>& cc, std::vector<uint8_t>& desc, std::vector<int32_t>& word, std::vector<float>& weight)
{
    int n = 1, width = 1;
    for (int l = 1; l <= levels; l++) { width *= k; n += width; }
    cb.assign(n, 0); cc.assign(n, 0); desc.resize((size_t)n * 32); word.assign(n, -1); weight.assign(n, 0.f);
    for (auto& v : desc) v = (uint8_t)rng();
    int next = 1, words = 0;
    std::vector<int> level(n, 0);
    for (int i = 0; i < n; i++) {
        if (level[i] < levels && next + k <= n) { cb[i] = next; cc[i] = k; for (int c = 0; c < k; c++) level[next + c] = level[i] + 1; next += k; }
        else { word[i] = words++; weight[i] = 0.5f + (float)(rng() % 100) / 100.f; }
    }
    hs_vocab_tree T{ n, levels, cb.data(), cc.data(), desc.data(), word.data(), weight.data(), nullptr };
    hs_vocab* v = nullptr;
    return hs_vocab_from_tree(&T, k, &v) == HS_OK ? v : nullptr;
}

static std::vector<uint8_t> slurp(const std::string& p) { std::vector<uint8_t> b; FILE* f = fopen(p.c_str(), "rb"); if (!f) return b; int c; while ((c = fgetc(f)) != EOF) b.push_back((uint8_t)c); fclose(f); return b; }
static void spit(const std::string& p, const std::vector<uint8_t>& b) { FILE* f = fopen(p.c_str(), "wb"); if (f) { if (!b.empty()) fwrite(b.data(), 1, b.size(), f); fclose(f); } }


// ---- the thirteen host-pointer entry points that lay their device side out with HsStage (hs_internal.h), on ONE handle in a random order: the
// scratch arena grows with the largest call so far and smaller calls reuse it.  Every count is drawn from [0, 300] (0 and 1 forced), every host
// buffer is a std::vector of exactly the documented size (a copy of the wrong length is a sanitizer report), the optional inputs are toggled.
// What this cannot see: an overrun that stays inside the arena (a piece running into its neighbour, or into HS_STAGE_SLACK) is no sanitizer report.
static int cnt(int forced) { return forced >= 0 ? forced : rnd(0, 300); }
static std::vector<hs_keypoint> rand_kps(int n, int w, int h)
{
    std::vector<hs_keypoint> k(n);
    for (auto& q : k) q = hs_keypoint{ (float)rnd(0, w), (float)rnd(0, h), 31.f, (float)rnd(0, 359), 1.f, rnd(0, 7) };
    return k;
}
static std::vector<uint8_t> rand_bytes(size_t n) { std::vector<uint8_t> b(n); for (auto& v : b) v = (uint8_t)rng(); return b; }
static std::vector<hs_landmark> rand_lms(int n)
{
    std::vector<hs_landmark> lm(n);
    for (auto& m : lm) { memset(&m, 0, sizeof(m)); m.pos[0] = (float)rnd(-3, 3); m.pos[2] = 5.f; m.size = 0.5f; m.max_dist = 100.f; m.assoc_kp = -1; }
    return lm;
}
// a feature vector over n features: `nn` nodes with ascending ids, CSR lists of feature indices
static void rand_featvec(int n, int nn, std::vector<int32_t>& id, std::vector<int32_t>& ptr, std::vector<int32_t>& idx)
{
    if (n == 0) nn = 0;                                      // (nodes need a non-null index list: the first node gets an entry)
    id.resize(nn); ptr.assign((size_t)nn + 1, 0); idx.clear();
    for (int a = 0, v = 0; a < nn; a++) { v += rnd(1, 3); id[a] = v; }
    for (int a = 0; a < nn; a++) { const int m = rnd(a == 0, 3); for (int j = 0; j < m; j++) idx.push_back(rnd(0, n - 1)); ptr[a + 1] = (int32_t)idx.size(); }
}
// CSR offsets of L lists with 0..3 entries each
static std::vector<int64_t> rand_csr(int L) { std::vector<int64_t> o((size_t)L + 1, 0); for (int i = 0; i < L; i++) o[i + 1] = o[i] + rnd(0, 3); return o; }

// alone: nothing else runs (the live-allocation count and the cache are this call's own to check)
static int staged_sweep(int rounds, bool alone = true)
{
    hs_orb_params p; hs_orb_default_params(&p); p.nfeatures = 300;
    hs_orb *ex = nullptr, *h = nullptr;                          // ex extracts and publishes frames, h is the ONE handle of the sweep
    const Live before = live_now();
    CHECK(hs_orb_create(&p, 0, &ex) == HS_OK && hs_orb_create(&p, 0, &h) == HS_OK);
    const int w = 320, hh = 240;
    const std::vector<uint8_t> img = rand_bytes((size_t)w * hh);
    CHECK(hs_orb_reserve(ex, w, hh, 1) == HS_OK);
    const int cap = hs_orb_max_keypoints(ex);
    CHECK(cap >= 300);
    { std::vector<hs_keypoint> k(cap); std::vector<uint8_t> d((size_t)cap * 32); int32_t n = 0; CHECK(hs_orb_extract(ex, img.data(), w, hh, w, k.data(), d.data(), cap, &n) == HS_OK); }
    hs_frame_view F0; memset(&F0, 0, sizeof(F0));
    F0.fx = F0.fy = 300.f; F0.cx = 160.f; F0.cy = 120.f; F0.max_x = (float)w; F0.max_y = (float)hh; F0.size_ref = 31.f; F0.Rcw[0] = F0.Rcw[4] = F0.Rcw[8] = 1.f; F0.mbf = 40.f; F0.sensor = 1;
    hs_proj_params pp; memset(&pp, 0, sizeof(pp)); pp.th = 3.f; pp.score_threshold = 100.f; pp.second_best_ratio = 0.8f; pp.frac_smaller = 0.5f; pp.frac_larger = 1.5f;
    std::vector<int32_t> cb, cc, word; std::vector<uint8_t> vdesc; std::vector<float> weight;
    { hs_vocab* v = make_vocab(3, 3, cb, cc, vdesc, word, weight); CHECK(v != nullptr); hs_vocab_destroy(v); }
    const hs_lm_entry_params ep{ 2.0f, 0.5f };
    const float Scw[12] = { 2, 0, 0, 0.1f, 0, 2, 0, 0.2f, 0, 0, 2, 0.3f }, R12[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, t12[3] = { 0.1f, 0.f, 0.f }, F12[9] = { 0, 0, 0, 0, 0, -1, 0, 1, 0 };
    int calls = 0;
    for (int r = 0; r < rounds; r++) {
        int order[14]; for (int i = 0; i < 14; i++) order[i] = i;
        for (int i = 13; i > 0; i--) std::swap(order[i], order[rnd(0, i)]);
        for (int oi = 0; oi < 14; oi++) {
            const int forced = r == 0 ? 0 : (r == 1 ? 1 : -1);       // the first two rounds: every count 0, then every count 1
            const int n = cnt(forced), n2 = cnt(forced), L = cnt(forced);
            const bool opt_a = rnd(0, 1), opt_b = rnd(0, 1), opt_c = rnd(0, 1);
            const std::vector<hs_keypoint> k1 = rand_kps(n, w, hh), k2 = rand_kps(n2, w, hh);
            const std::vector<uint8_t> d1 = rand_bytes((size_t)n * 32), d2 = rand_bytes((size_t)n2 * 32);
            const std::vector<float> uR(n, -1.f); const std::vector<int32_t> obs(n, -1);
            hs_frame_view F = F0; F.n = n; F.kps = k1.data(); F.desc = d1.data(); F.uR = opt_a ? uR.data() : nullptr; F.kp_lm_obs = opt_b ? obs.data() : nullptr;
            hs_frame_view G = F0; G.n = n2; G.kps = k2.data(); G.desc = d2.data();
            pp.use_stereo = opt_a;
            const std::vector<hs_landmark> lms = rand_lms(L);
            std::vector<int32_t> mi(L); std::vector<float> md(L); int32_t nm = -1;
            hip_stub_zero_device();
            int st = HS_OK;
            switch (order[oi]) {
            case 0: st = hs_search_by_projection(h, &F, lms.data(), L, &pp, mi.data(), md.data(), &nm); break;
            case 1: {                                                // a published frame of max(n, 1) keypoints
                const int nf = std::max(n, 1);
                const std::vector<hs_keypoint> kf = rand_kps(nf, w, hh); const std::vector<float> uf(nf, -1.f); const std::vector<int32_t> of(nf, -1);
                hs_frame_token tok = 0;
                CHECK(hs_frame_publish(ex, 0, kf.data(), nf, &tok) == HS_OK);
                hs_frame_view P = F0; P.n = nf; P.uR = opt_a ? uf.data() : nullptr; P.kp_lm_obs = opt_b ? of.data() : nullptr;
                st = hs_search_by_projection_frame(h, tok, &P, lms.data(), L, &pp, mi.data(), md.data(), &nm);
                CHECK(hs_frame_release(0, tok) == HS_OK);
                break; }
            case 2: {                                                // "device" pointers are host memory under the stub; n, L >= 1 by contract
                const int nf = std::max(n, 1), Lf = std::max(L, 1);
                const std::vector<hs_keypoint> kf = rand_kps(nf, w, hh); const std::vector<uint8_t> df = rand_bytes((size_t)nf * 32);
                const std::vector<float> uf(nf, -1.f); const std::vector<int32_t> of(nf, -1); const std::vector<hs_landmark> lf = rand_lms(Lf);
                std::vector<int32_t> mf(Lf); std::vector<float> mdf(Lf);
                hs_frame_view P = F0; P.n = nf; P.kps = kf.data(); P.desc = df.data(); P.uR = opt_a ? uf.data() : nullptr; P.kp_lm_obs = opt_b ? of.data() : nullptr;
                st = hs_search_by_projection_device(h, &P, lf.data(), Lf, &pp, mf.data(), mdf.data(), &nm, nullptr);
                break; }
            case 3: { std::vector<int8_t> cell((size_t)n * 2); st = hs_frame_grid(h, &F, cell.data()); break; }
            case 4: { std::vector<uint8_t> taken(n, 0); st = hs_search_by_projection_sim3(h, &F, Scw, lms.data(), L, 10, 50.f, taken.data(), mi.data(), &nm); break; }
            case 5: {
                const std::vector<hs_landmark> l1 = rand_lms(n), l2 = rand_lms(n2); std::vector<int32_t> m12(n);
                st = hs_search_by_sim3(h, &F, l1.data(), &G, l2.data(), 1.1f, R12, t12, 7.5f, 100.f, m12.data(), &nm);
                break; }
            case 6: case 7: {                                       // bow_host through both of its doors
                std::vector<int32_t> id1, p1, i1, id2, p2, i2, m12(n);
                rand_featvec(n, cnt(forced), id1, p1, i1); rand_featvec(n2, cnt(forced), id2, p2, i2);
                const std::vector<uint8_t> keep1(n, 1), keep2(n2, 1);
                if (order[oi] == 6)
                    st = hs_search_by_bow_ex(h, k1.data(), d1.data(), n, id1.data(), p1.data(), i1.data(), (int)id1.size(), k2.data(), d2.data(), n2, id2.data(), p2.data(), i2.data(), (int)id2.size(),
                                             opt_a ? keep1.data() : nullptr, opt_b ? keep2.data() : nullptr, opt_c ? F12 : nullptr, 31.f, 1.f, 50.f, 0.6f, 1, m12.data(), &nm);
                else
                    st = hs_search_by_bow_legacy(h, k1.data(), d1.data(), n, id1.data(), p1.data(), i1.data(), (int)id1.size(), k2.data(), d2.data(), n2, id2.data(), p2.data(), i2.data(), (int)id2.size(),
                                                 opt_a ? keep1.data() : nullptr, opt_b ? keep2.data() : nullptr, 50.f, 0.6f, 1, m12.data(), &nm);
                break; }
            case 8: { std::vector<float> prev((size_t)n * 2, 10.f); std::vector<int32_t> m12(n); st = hs_search_for_initialization(h, k1.data(), d1.data(), n, &G, prev.data(), 100, 50.f, 0.9f, m12.data(), &nm); break; }
            case 9: {
                const std::vector<int32_t> orig(cb.size(), 0);
                const hs_vocab_tree T{ (int32_t)cb.size(), 3, cb.data(), cc.data(), vdesc.data(), word.data(), weight.data(), opt_a ? orig.data() : nullptr };
                std::vector<int32_t> wi(n), ni(n); std::vector<float> wt(n);
                st = hs_bow_transform(h, &T, d1.data(), n, 1, wi.data(), wt.data(), ni.data());
                break; }
            case 10: { std::vector<int32_t> bi(n), bd(n), sd(n); st = hs_hamming_knn2(h, d1.data(), n, d2.data(), n2, bi.data(), bd.data(), sd.data()); break; }
            case 11: {
                const std::vector<int64_t> off = rand_csr(L); const std::vector<uint8_t> dd = rand_bytes((size_t)off[L] * 32); std::vector<int32_t> best(L), med(L);
                st = hs_landmark_best_descriptors(h, off.data(), dd.data(), L, best.data(), med.data());
                break; }
            case 12: {
                const std::vector<int64_t> oo = rand_csr(L), od = rand_csr(L);
                const std::vector<hs_lm_entry_in> ent(L); const std::vector<hs_lm_obs> ob((size_t)oo[L]); const std::vector<uint8_t> dd = rand_bytes((size_t)od[L] * 32);
                std::vector<float> nrm((size_t)L * 3), mind(L), maxd(L), mean(L), size(L); std::vector<int32_t> best(L), med(L), flags(L);
                st = hs_landmark_update_entries(h, &ep, L, ent.data(), oo.data(), ob.data(), od.data(), dd.data(), nrm.data(), mind.data(), maxd.data(), mean.data(), size.data(),
                                                best.data(), med.data(), flags.data());
                break; }
            case 13: {
                std::vector<int32_t> wd(n), ow(n); const std::vector<float> wt(n, 1.f); std::vector<double> ov(n); int32_t m = -1;
                for (auto& v : wd) v = rnd(0, 50);
                st = hs_bow_vector(h, wd.data(), wt.data(), n, ow.data(), ov.data(), &m);
                CHECK(m == 0);
                break; }
            }
            if (st != HS_OK) { printf("staged sweep: entry point %d, n %d n2 %d L %d: status %d (%s)\n", order[oi], n, n2, L, st, hs_orb_last_error(h)); return 1; }
            calls++;
        }
    }
    hs_orb_destroy(ex); hs_orb_destroy(h);
    if (alone) {
        CHECK(hs_frame_cache_clear(0) == HS_OK);                 // (the published frames belong to the cache, not to a handle)
        CHECK(same_live(before));
    }
    return calls > 0 ? 0 : 1;
}

// ---- the key-frame graph, the local map and the pose optimiser by host pointers, the *_work_bytes functions, and the `_device` forms of the
// tracking, reference-key-frame and key-frame stages ("device" pointers are host memory under the stub; every work area is a vector of exactly
// *_work_bytes), on ONE handle in a random order, in the style of staged_sweep: counts from [0, 300] with 0 and 1 forced in the first two rounds,
// every host buffer a std::vector of exactly the documented size, optional arguments toggled, the refusals on the way.
struct Table {
    std::vector<int64_t> off, kf_id; std::vector<int32_t> kf, oct, nobs; std::vector<uint8_t> lm_bad, kf_bad;
    hs_kf_table T;
};
static void rand_table(Table& t, int L, int n_kf)
{
    t.off.assign((size_t)L + 1, 0); t.kf.clear(); t.oct.clear();
    for (int l = 0; l < L; l++) {                               // ascending slots within a landmark
        const int m = n_kf > 0 ? rnd(0, std::min(3, n_kf)) : 0;
        for (int j = 0, s = rnd(0, std::max(n_kf - m, 0)); j < m; j++, s++) { t.kf.push_back(s); t.oct.push_back(rnd(0, 7)); }
        t.off[l + 1] = (int64_t)t.kf.size();
    }
    t.nobs.resize(L); t.lm_bad.resize(L); t.kf_bad.resize(n_kf); t.kf_id.resize(n_kf);
    for (int l = 0; l < L; l++) { t.nobs[l] = (int32_t)(t.off[l + 1] - t.off[l]) + rnd(0, 1); t.lm_bad[l] = rnd(0, 9) == 0; }
    for (int k = 0; k < n_kf; k++) { t.kf_bad[k] = rnd(0, 9) == 0; t.kf_id[k] = 100 + k; }
    t.T = hs_kf_table{ L, n_kf, t.off.data(), t.kf.data(), t.oct.data(), t.lm_bad.data(), t.nobs.data(), t.kf_bad.data(), t.kf_id.data() };
}
// Q lists of 0..max_len indices below `bound` (none when bound is 0)
static void rand_lists(int Q, int bound, int max_len, std::vector<int64_t>& off, std::vector<int32_t>& idx)
{
    off.assign((size_t)Q + 1, 0); idx.clear();
    for (int q = 0; q < Q; q++) { const int m = bound > 0 ? rnd(0, max_len) : 0; for (int j = 0; j < m; j++) idx.push_back(rnd(0, bound - 1)); off[q + 1] = (int64_t)idx.size(); }
}

static int map_sweep(int rounds, bool alone = true)
{
    hs_orb_params p; hs_orb_default_params(&p); p.nfeatures = 300;
    hs_orb* h = nullptr;
    const Live before = live_now();
    CHECK(hs_orb_create(&p, 0, &h) == HS_OK);
    hs_track_params tp; memset(&tp, 0, sizeof(tp));
    tp.th_motion = 15.f; tp.th_motion_wide = 30.f; tp.n_min_matches = 20; tp.th_local = 3.f; tp.nnratio_motion = 0.9f; tp.nnratio_local = 0.8f; tp.th_high = 100.f; tp.sigma_ref = 1.f;
    tp.n_max_local_keyframes = 80; tp.n_neighbor_keyframes = 10;
    hs_keyframe_params kp; memset(&kp, 0, sizeof(kp)); kp.frame_id = 100; kp.last_keyframe_id = 10; kp.max_KF_interval = 30; kp.th_depth = 40.f; kp.n_min_points = 100; kp.ok_override = -1;
    const hs_lm_entry_params ep{ 2.0f, 0.5f };
    // the work-size functions alone: monotone in every argument over the sweep's range, and 0 never crashes
    for (int i = 0; i < 50; i++) {
        const int n = rnd(0, 300), m = rnd(0, 300), L = rnd(0, 300), c = rnd(0, 300);
        CHECK(hs_local_points_work_bytes(L) <= hs_local_points_work_bytes(L + 1024) && hs_local_map_work_bytes(L) >= hs_local_points_work_bytes(L));
        CHECK(hs_track_work_bytes(n, m, L, c) <= hs_track_work_bytes(n + 64, m, L + 64, c) && hs_track_refkf_work_bytes(n, c, L) <= hs_track_refkf_work_bytes(n + 64, c, L + 64));
        CHECK(hs_keyframe_work_bytes(n, m, c) <= hs_keyframe_work_bytes(n + 64, m + 64, c + 64) && hs_pose_work_bytes(n, (int64_t)n * m) == 0);
    }
    int calls = 0, refused = 0;
    for (int r = 0; r < rounds; r++) {
        int order[8]; for (int i = 0; i < 8; i++) order[i] = i;
        for (int i = 7; i > 0; i--) std::swap(order[i], order[rnd(0, i)]);
        for (int oi = 0; oi < 8; oi++) {
            const int forced = r == 0 ? 0 : (r == 1 ? 1 : -1);
            const int L = cnt(forced), n_kf = cnt(forced), Q = cnt(forced) % 8, n = cnt(forced);
            const bool opt_a = rnd(0, 1), opt_b = rnd(0, 1);
            Table t; rand_table(t, L, n_kf);
            hip_stub_zero_device();
            int st = HS_OK;
            switch (order[oi]) {
            case 0: {                                            // hs_kf_votes: weights and the self ids optional, cap 0 = no list
                std::vector<int64_t> qo; std::vector<int32_t> ql; rand_lists(Q, L, 40, qo, ql);
                const std::vector<int64_t> self(Q, -1); const int cap = opt_b ? 0 : rnd(1, 12);
                std::vector<int32_t> w((size_t)Q * n_kf), ms(Q), mc(Q), os((size_t)Q * cap), ow((size_t)Q * cap), no(Q);
                st = hs_kf_votes(h, &t.T, Q, qo.data(), ql.data(), opt_a ? self.data() : nullptr, rnd(0, 1), 2, opt_a ? w.data() : nullptr, ms.data(), mc.data(), os.data(), ow.data(), cap, no.data());
                if (st == HS_OK && Q > 0) {                      // the refusals: offsets that decrease, a landmark outside the table; no output touched
                    std::vector<int64_t> bad = qo; bad[Q] = -1;
                    ms.assign(Q, 77);
                    CHECK(hs_kf_votes(h, &t.T, Q, bad.data(), ql.data(), nullptr, 0, 2, nullptr, ms.data(), mc.data(), os.data(), ow.data(), cap, no.data()) == HS_ERR_INVALID && ms[0] == 77);
                    if (!ql.empty()) { std::vector<int32_t> out_of = ql; out_of[0] = L; CHECK(hs_kf_votes(h, &t.T, Q, qo.data(), out_of.data(), nullptr, 0, 2, nullptr, ms.data(), mc.data(), os.data(), ow.data(), cap, no.data()) == HS_ERR_INVALID); refused++; }
                    if (L > 0) { Table u = t; u.off[L] = u.off[L - 1] - 1; u.T.lm_obs_offsets = u.off.data(); CHECK(hs_kf_votes(h, &u.T, Q, qo.data(), ql.data(), nullptr, 0, 2, nullptr, ms.data(), mc.data(), os.data(), ow.data(), cap, no.data()) == HS_ERR_INVALID); }
                    refused += 2;
                }
                break; }
            case 1: {                                            // hs_kf_redundancy: mono (no depths) or not
                const int Cn = Q; std::vector<int64_t> co; std::vector<int32_t> il; rand_lists(Cn, L, 60, co, il);
                std::vector<int32_t> slot(Cn), io(il.size()), nm(Cn), nr(Cn); std::vector<float> thd(Cn, 40.f), dep(il.size(), 10.f); std::vector<uint8_t> cull(Cn);
                for (auto& v : slot) v = n_kf > 0 ? rnd(0, n_kf - 1) : 0;
                st = hs_kf_redundancy(h, &t.T, Cn, slot.data(), thd.data(), co.data(), il.data(), io.data(), opt_a ? nullptr : dep.data(), opt_a, 3, 0.9f, nm.data(), nr.data(), cull.data());
                if (st == HS_OK && Cn > 0) {
                    std::vector<int64_t> bad = co; bad[0] = 1; if (Cn > 1) bad[1] = 0; else bad[1] = 0;      // decreasing (or starting above its end)
                    nm.assign(Cn, 77);
                    CHECK(hs_kf_redundancy(h, &t.T, Cn, slot.data(), thd.data(), bad.data(), il.data(), io.data(), dep.data(), 0, 3, 0.9f, nm.data(), nr.data(), cull.data()) == HS_ERR_INVALID && nm[0] == 77);
                    bad = co; bad[Cn] = -5;
                    CHECK(hs_kf_redundancy(h, &t.T, Cn, slot.data(), thd.data(), bad.data(), il.data(), io.data(), dep.data(), 0, 3, 0.9f, nm.data(), nr.data(), cull.data()) == HS_ERR_INVALID);
                    if (!il.empty()) { std::vector<int32_t> out_of = il; out_of.back() = -1; CHECK(hs_kf_redundancy(h, &t.T, Cn, slot.data(), thd.data(), co.data(), out_of.data(), io.data(), dep.data(), 0, 3, 0.9f, nm.data(), nr.data(), cull.data()) == HS_ERR_INVALID); }
                    refused += 2;
                }
                break; }
            case 2: {                                            // hs_local_keyframes
                const int nc = opt_a ? 10 : rnd(0, 12);
                std::vector<int32_t> w(n_kf), neigh((size_t)n_kf * nc, -1), parent(n_kf, -1); int32_t nl = -1; std::vector<uint8_t> local(n_kf);
                for (auto& v : w) v = rnd(0, 3);
                for (auto& v : neigh) v = rnd(-1, n_kf - 1);
                for (auto& v : parent) v = rnd(-1, n_kf - 1);
                st = hs_local_keyframes(h, n_kf, w.data(), t.kf_bad.data(), neigh.data(), nc, parent.data(), opt_b ? -1 : 80, std::min(nc, 10), local.data(), &nl);
                if (st == HS_OK) {
                    CHECK(hs_local_keyframes(h, n_kf, w.data(), t.kf_bad.data(), neigh.data(), nc, parent.data(), 80, nc + 1, local.data(), &nl) == HS_ERR_INVALID);
                    if (n_kf > 0) { parent[n_kf - 1] = n_kf; CHECK(hs_local_keyframes(h, n_kf, w.data(), t.kf_bad.data(), neigh.data(), nc, parent.data(), 80, 0, local.data(), &nl) == HS_ERR_INVALID); }
                    refused++;
                }
                break; }
            case 3: {                                            // hs_local_points
                const int cap = opt_a ? 0 : cnt(forced);
                std::vector<uint8_t> local(n_kf, 1), rem(n); std::vector<int32_t> flm(n), sel(cap); int32_t ns = -1;
                for (auto& v : flm) v = rnd(-1, L - 1);
                st = hs_local_points(h, &t.T, local.data(), flm.data(), n, rem.data(), sel.data(), cap, &ns);
                if (st == HS_OK && n > 0) { flm[0] = L; CHECK(hs_local_points(h, &t.T, local.data(), flm.data(), n, rem.data(), sel.data(), cap, &ns) == HS_ERR_INVALID); refused++; }
                break; }
            case 4: {                                            // hs_pose_optimize: Q of 0, 1 and several; problems with fewer than 3 edges among them
                std::vector<int64_t> eo((size_t)Q + 1, 0);
                for (int q = 0; q < Q; q++) eo[q + 1] = eo[q] + (forced >= 0 ? forced : rnd(0, 40));
                std::vector<hs_pose_problem> pr(Q); std::vector<hs_pose_edge> ed((size_t)eo[Q]); std::vector<uint8_t> outl((size_t)eo[Q], 0); std::vector<hs_pose_result> res(Q);
                for (auto& q : pr) { memset(&q, 0, sizeof(q)); q.Tcw[0] = q.Tcw[5] = q.Tcw[10] = q.Tcw[15] = 1.f; q.fx = q.fy = 300.f; q.cx = 160.f; q.cy = 120.f; q.bf = 40.f; }
                for (auto& e : ed) e = hs_pose_edge{ { (float)rnd(-3, 3), (float)rnd(-3, 3), 5.f }, (float)rnd(0, 320), (float)rnd(0, 240), opt_a ? -1.f : 100.f, 1.f, 0 };
                st = hs_pose_optimize(h, Q, pr.data(), eo.data(), ed.data(), outl.data(), res.data());
                if (st == HS_OK && Q > 0) { eo[Q] = -1; CHECK(hs_pose_optimize(h, Q, pr.data(), eo.data(), ed.data(), outl.data(), res.data()) == HS_ERR_INVALID); refused++; }
                break; }
            case 5: case 6: {                                    // the tracking chain: the two stages, or the fused call (n, n_last, L, cap >= 1 by contract)
                const int nf = std::max(n, 1), nlast = std::max(cnt(forced), 1), Lf = std::max(L, 1), kf = std::max(n_kf, 1), cap = std::max(cnt(forced), 1);
                Table u; rand_table(u, Lf, kf);
                const std::vector<hs_keypoint> k1 = rand_kps(nf, 320, 240), kl = rand_kps(nlast, 320, 240); const std::vector<uint8_t> d1 = rand_bytes((size_t)nf * 32);
                const std::vector<float> uR(nf, -1.f), Tp(16, 0.f); const std::vector<hs_landmark> lms = rand_lms(Lf);
                std::vector<int32_t> last_lm(nlast, -1), neigh((size_t)kf * 10, -1), parent(kf, -1);
                hs_frame_view F; memset(&F, 0, sizeof(F));
                F.fx = F.fy = 300.f; F.cx = 160.f; F.cy = 120.f; F.max_x = 320.f; F.max_y = 240.f; F.size_ref = 31.f; F.mbf = 40.f; F.sensor = opt_a; F.n = nf; F.kps = k1.data(); F.desc = d1.data();
                F.uR = opt_a ? uR.data() : nullptr;
                std::vector<int32_t> s_lm(nf, -1), s_nm(1, 0), s_obs(nf, -1); std::vector<uint8_t> s_outl(nf, 0);
                const hs_track_state S{ s_lm.data(), s_outl.data(), s_nm.data(), s_obs.data() };
                std::vector<hs_pose_view> pv(2); std::vector<hs_pose_problem> prob(2); std::vector<hs_landmark> last_rec(nlast), loc_lms(cap);
                std::vector<int32_t> ni(nlast), wi(nlast), nn(1), wn(1), opv(nlast), ne_m(2), ne_l(1), lw(kf), lms_slot(1), lmc(1), lnl(1), lsel(cap), lns(1), lmi(cap), lnm(1);
                std::vector<float> nd(nlast), wd(nlast), lmd(cap); std::vector<hs_pose_edge> em(nf), el(nf); std::vector<uint8_t> om(nf), ol(nf), lloc(kf), lrem(nf);
                std::vector<hs_pose_result> pm(1), pl(1); std::vector<hs_track_result> tr(1);
                const hs_local_map_out lo{ lw.data(), lms_slot.data(), lmc.data(), lloc.data(), lnl.data(), lrem.data(), lsel.data(), lns.data(), loc_lms.data(), lmi.data(), lmd.data(), lnm.data() };
                const hs_track_out O{ pv.data(), prob.data(), last_rec.data(), ni.data(), nd.data(), nn.data(), wi.data(), wd.data(), wn.data(), opv.data(), em.data(), om.data(), ne_m.data(), pm.data(), lo,
                                      el.data(), ol.data(), ne_l.data(), pl.data(), tr.data() };
                std::vector<uint8_t> work(hs_track_work_bytes(nf, nlast, Lf, cap));
                CHECK(!work.empty());
                if (order[oi] == 5) {
                    st = hs_track_motion_model_device(h, &F, Tp.data(), kl.data(), last_lm.data(), nlast, &u.T, lms.data(), &tp, &S, &O, work.data(), nullptr);
                    if (st == HS_OK) st = hs_track_local_map_device(h, &F, pm[0].Tcw, &u.T, lms.data(), neigh.data(), 10, parent.data(), cap, &tp, &S, &O, work.data(), nullptr);
                } else
                    st = hs_track_frame_device(h, &F, Tp.data(), kl.data(), last_lm.data(), nlast, &u.T, lms.data(), neigh.data(), 10, parent.data(), cap, &tp, &S, &O, work.data(), nullptr);
                if (st == HS_OK) {                               // refused before the first launch: no work area, a frame without keypoints, a state with a hole
                    CHECK(hs_track_frame_device(h, &F, Tp.data(), kl.data(), last_lm.data(), nlast, &u.T, lms.data(), neigh.data(), 10, parent.data(), cap, &tp, &S, &O, nullptr, nullptr) == HS_ERR_INVALID);
                    hs_frame_view F0 = F; F0.n = 0;
                    CHECK(hs_track_motion_model_device(h, &F0, Tp.data(), kl.data(), last_lm.data(), nlast, &u.T, lms.data(), &tp, &S, &O, work.data(), nullptr) == HS_ERR_INVALID);
                    hs_track_state S0 = S; S0.kp_outl = nullptr;
                    CHECK(hs_track_local_map_device(h, &F, pm[0].Tcw, &u.T, lms.data(), neigh.data(), 10, parent.data(), cap, &tp, &S0, &O, work.data(), nullptr) == HS_ERR_INVALID);
                    CHECK(hs_track_local_map_device(h, &F, pm[0].Tcw, &u.T, lms.data(), neigh.data(), 10, parent.data(), 0, &tp, &S, &O, work.data(), nullptr) == HS_ERR_INVALID);
                    refused += 4;
                    // the replay, the frame views and the discard on their own
                    std::vector<uint8_t> aw(hs_track_work_bytes(nf, 0, Lf, 0));
                    st = hs_frame_associate_device(h, nf, Lf, s_lm.data(), s_outl.data(), s_nm.data(), nlast, opv.data(), last_lm.data(), aw.data(), nullptr);
                    if (st == HS_OK) st = hs_frame_views_device(h, nf, s_lm.data(), s_outl.data(), s_nm.data(), &u.T, opt_b, s_obs.data(), nullptr);
                    if (st == HS_OK) st = hs_track_discard_device(h, opt_b ? HS_TRACK_LOCAL : HS_TRACK_MOTION, em.data(), ne_l.data(), nf, om.data(), pm.data(), &u.T, F.sensor, s_lm.data(), s_outl.data(), s_nm.data(), lnm.data(), nullptr);
                    if (st == HS_OK) st = hs_pose_views_device(h, Tp.data(), pv.data(), nullptr);
                    CHECK(hs_track_discard_device(h, 2, em.data(), ne_l.data(), nf, om.data(), pm.data(), &u.T, F.sensor, s_lm.data(), s_outl.data(), s_nm.data(), lnm.data(), nullptr) == HS_ERR_INVALID);
                }
                break; }
            case 7: {                                            // the reference-key-frame pair, then the key-frame stages one by one and fused, then the entry update they feed
                const int nf = std::max(n, 1), Lf = std::max(L, 1), kf = std::max(n_kf, 1), kf_cap = std::max(cnt(forced), 1), new_cap = opt_a ? 0 : std::max(cnt(forced), 1);
                Table u; rand_table(u, Lf, kf);
                std::vector<int64_t> ko((size_t)kf + 1, 0);
                for (int k = 0; k < kf; k++) ko[k + 1] = ko[k] + rnd(0, 5);
                const int total = (int)ko[kf];
                const std::vector<hs_keypoint> kk = rand_kps(std::max(total, 1), 320, 240), k1 = rand_kps(nf, 320, 240);
                const std::vector<uint8_t> kd = rand_bytes((size_t)std::max(total, 1) * 32), d1 = rand_bytes((size_t)nf * 32);
                const std::vector<int32_t> knode(std::max(total, 1), 3), klm(std::max(total, 1), -1), fnode(nf, 3); const std::vector<float> kw(std::max(total, 1), 1.f), fw(nf, 1.f);
                const hs_kf_features K{ kf, ko.data(), kk.data(), kd.data(), knode.data(), klm.data(), opt_b ? kw.data() : nullptr };
                std::vector<int32_t> slot(1, rnd(-1, kf)), mkf(kf_cap), opv(nf), opl(nf), nm(1);
                st = hs_search_by_bow_kf_device(h, &K, slot.data(), &u.T, k1.data(), d1.data(), fnode.data(), opt_b ? fw.data() : nullptr, nf, 50.f, 0.7f, mkf.data(), kf_cap, opv.data(), opl.data(), nm.data(), nullptr, nullptr);
                if (st != HS_OK) break;
                CHECK(hs_search_by_bow_kf_device(h, &K, slot.data(), &u.T, k1.data(), d1.data(), fnode.data(), nullptr, nf, 50.f, 0.7f, mkf.data(), 0, opv.data(), opl.data(), nm.data(), nullptr, nullptr) == HS_ERR_INVALID);
                CHECK(hs_search_by_bow_kf_device(h, nullptr, slot.data(), &u.T, k1.data(), d1.data(), fnode.data(), nullptr, nf, 50.f, 0.7f, mkf.data(), kf_cap, opv.data(), opl.data(), nm.data(), nullptr, nullptr) == HS_ERR_INVALID);
                std::vector<int32_t> s_lm(nf, -1), s_nm(1, 0), s_obs(nf, -1); std::vector<uint8_t> s_outl(nf, 0);
                const hs_track_state S{ s_lm.data(), s_outl.data(), s_nm.data(), s_obs.data() };
                std::vector<uint8_t> vw(hs_track_refkf_work_bytes(nf, kf_cap, Lf));
                st = hs_frame_associate_views_device(h, nf, Lf, s_lm.data(), s_outl.data(), s_nm.data(), opv.data(), opl.data(), vw.data(), nullptr);
                if (st != HS_OK) break;
                CHECK(hs_frame_associate_views_device(h, nf, Lf, s_lm.data(), s_outl.data(), s_nm.data(), opv.data(), opl.data(), nullptr, nullptr) == HS_ERR_INVALID);
                hs_frame_view F; memset(&F, 0, sizeof(F));
                F.fx = F.fy = 300.f; F.cx = 160.f; F.cy = 120.f; F.max_x = 320.f; F.max_y = 240.f; F.size_ref = 31.f; F.mbf = 40.f; F.sensor = 1; F.n = nf; F.kps = k1.data(); F.desc = d1.data();
                const std::vector<float> depth(nf, 10.f), Tcw(16, 0.f);
                std::vector<hs_keyframe_result> res(1); std::vector<hs_pose_view> pv(1); std::vector<int32_t> nv(new_cap), lmi(new_cap); std::vector<float> np((size_t)new_cap * 3);
                std::vector<hs_lm_entry_in> ent(new_cap); std::vector<hs_lm_obs> obs(new_cap); std::vector<int64_t> oo((size_t)new_cap + 1), od((size_t)new_cap + 1); std::vector<uint8_t> nd((size_t)new_cap * 32);
                std::vector<hs_landmark> lms((size_t)Lf + new_cap);
                const hs_keyframe_out KO{ res.data(), pv.data(), nv.data(), np.data(), ent.data(), obs.data(), oo.data(), od.data(), nd.data(), lmi.data(), opt_b ? lms.data() : nullptr, opt_b ? Lf + new_cap : 0 };
                std::vector<hs_track_result> tr(1); std::vector<int32_t> ref(1, -1);
                std::vector<uint8_t> kwork(hs_keyframe_work_bytes(nf, kf, new_cap));
                CHECK(!kwork.empty());
                st = hs_keyframe_reference_device(h, nf, &S, &u.T, ref.data(), res.data(), kwork.data(), nullptr);
                if (st == HS_OK) st = hs_keyframe_gate_device(h, tr.data(), &kp, res.data(), nullptr);
                if (st == HS_OK) st = hs_keyframe_clean_device(h, nf, &S, &u.T, res.data(), nullptr);
                if (st == HS_OK) st = hs_keyframe_need_device(h, nf, 1, depth.data(), &S, &u.T, &K, ref.data(), tr.data(), &kp, res.data(), nullptr);
                if (st == HS_OK) st = hs_keyframe_create_device(h, &F, depth.data(), Tcw.data(), &S, &u.T, &kp, new_cap, &KO, kwork.data(), nullptr);
                if (st == HS_OK) st = hs_keyframe_discard_device(h, nf, &S, res.data(), nullptr);
                if (st == HS_OK) st = hs_track_keyframe_device(h, &F, depth.data(), Tcw.data(), &u.T, &K, tr.data(), &kp, &S, ref.data(), new_cap, &KO, kwork.data(), nullptr);
                if (st != HS_OK) break;
                CHECK(hs_keyframe_gate_device(h, nullptr, &kp, res.data(), nullptr) == HS_ERR_INVALID);              // no track result and no override
                CHECK(hs_track_keyframe_device(h, &F, depth.data(), Tcw.data(), &u.T, &K, tr.data(), &kp, &S, ref.data(), new_cap, &KO, nullptr, nullptr) == HS_ERR_INVALID);
                CHECK(hs_track_keyframe_device(h, &F, depth.data(), Tcw.data(), &u.T, &K, tr.data(), &kp, &S, ref.data(), -1, &KO, kwork.data(), nullptr) == HS_ERR_INVALID);
                refused += 6;
                if (new_cap > 0) {
                    std::vector<float> nrm((size_t)new_cap * 3), a1(new_cap), a2(new_cap), a3(new_cap), a4(new_cap); std::vector<int32_t> b1(new_cap), b2(new_cap), b3(new_cap);
                    st = hs_landmark_update_entries_device(h, &ep, new_cap, ent.data(), oo.data(), obs.data(), od.data(), nd.data(), nrm.data(), a1.data(), a2.data(), a3.data(), a4.data(), b1.data(), b2.data(), b3.data(),
                                                           opt_b ? lms.data() : nullptr, opt_b ? lmi.data() : nullptr, opt_b ? Lf + new_cap : 0, nullptr);
                }
                break; }
            }
            if (st != HS_OK) { printf("map sweep: entry point %d, L %d n_kf %d Q %d n %d: status %d (%s)\n", order[oi], L, n_kf, Q, n, st, hs_orb_last_error(h)); return 1; }
            calls++;
        }
    }
    hs_orb_destroy(h);
    if (alone) CHECK(same_live(before));
    return calls > 0 && refused > 0 ? 0 : 1;
}

// ---- the place database's host code: the slot mirror, tombstones, the two regrow paths (slots from 1024, the entry pool from 65 536), the key-order
// upload of the first query after a change, clear and reuse, two databases alive at once, the refused vectors
static int place_add(hs_place_db* db, uint64_t key, int m, int n_words, int32_t* slot)
{
    std::vector<int32_t> w(m); std::vector<double> v(m);
    for (int i = 0, at = rnd(0, std::max(n_words - m, 0) / std::max(m, 1)); i < m; i++, at += 1 + rnd(0, std::max(n_words / std::max(m, 1) - 2, 0))) { w[i] = std::min(at, n_words - m + i); v[i] = 1.0 / m; }
    for (int i = 1; i < m; i++) if (w[i] <= w[i - 1]) w[i] = w[i - 1] + 1;
    return hs_place_db_add(db, key, w.data(), v.data(), m, slot);
}
static int place_queries(hs_place_db* db, int n_words, int want_slots)
{
    int32_t live = -1, slots = -1;
    CHECK(hs_place_db_size(db, &live, &slots) == HS_OK && slots == want_slots && live <= slots);
    const int qm = 30;
    std::vector<int32_t> qw(qm); std::vector<double> qv(qm, 1.0 / qm);
    for (int i = 0; i < qm; i++) qw[i] = i * (n_words / qm);
    std::vector<int32_t> neigh((size_t)slots * 10, -1), cand(std::max(slots, 1)), words(slots), best(slots); std::vector<float> score(slots), acc(slots); std::vector<uint8_t> excl(slots, 0);
    for (auto& v : neigh) v = rnd(-1, slots);                    // (out-of-range and tombstoned slots are ignored by contract)
    int32_t nc = -1;
    CHECK(hs_place_query_reloc(db, qw.data(), qv.data(), qm, neigh.data(), cand.data(), (int)cand.size(), &nc, words.data(), score.data(), acc.data(), best.data()) == HS_OK && nc >= 0);
    CHECK(hs_place_query_loop(db, qw.data(), qv.data(), qm, excl.data(), 0.f, nullptr, cand.data(), (int)cand.size(), &nc, nullptr, nullptr, nullptr, nullptr) == HS_OK && nc >= 0);
    CHECK(hs_place_query_reloc(db, qw.data(), qv.data(), 0, nullptr, cand.data(), (int)cand.size(), &nc, nullptr, nullptr, nullptr, nullptr) == HS_OK && nc == 0);
    return 0;
}
static int place_section(bool alone = true)
{
    hs_orb_params p; hs_orb_default_params(&p);
    hs_orb* h = nullptr;
    const Live before = live_now();
    CHECK(hs_orb_create(&p, 0, &h) == HS_OK);
    const int n_words = 5000;
    hs_place_db *db = nullptr, *db2 = nullptr;
    CHECK(hs_place_db_create(h, n_words, 1, &db) != HS_OK && db == nullptr);                    // only L1 scoring
    CHECK(hs_place_db_create(h, n_words, 0, &db) == HS_OK && hs_place_db_create(h, 100, 0, &db2) == HS_OK);
    CHECK(place_queries(db, n_words, 0) == 0);                                                   // an empty database answers
    int32_t slot = -1;
    // refused vectors: not ascending, a word >= n_words, a value <= 0 or not finite; nothing is stored
    { const int32_t w[3] = { 5, 4, 9 }; const double v[3] = { .3, .3, .4 }; CHECK(hs_place_db_add(db, 1, w, v, 3, &slot) == HS_ERR_INVALID); }
    { const int32_t w[3] = { 5, 5, 9 }; const double v[3] = { .3, .3, .4 }; CHECK(hs_place_db_add(db, 1, w, v, 3, &slot) == HS_ERR_INVALID); }
    { const int32_t w[2] = { 5, n_words }; const double v[2] = { .5, .5 }; CHECK(hs_place_db_add(db, 1, w, v, 2, &slot) == HS_ERR_INVALID); }
    { const int32_t w[2] = { 5, 6 }; const double v[2] = { .5, 0.0 }; CHECK(hs_place_db_add(db, 1, w, v, 2, &slot) == HS_ERR_INVALID); }
    { const int32_t w[2] = { 5, 6 }; const double v[2] = { -.5, .5 }; CHECK(hs_place_db_add(db, 1, w, v, 2, &slot) == HS_ERR_INVALID); }
    { const int32_t w[2] = { 5, 6 }; const double v[2] = { .5, std::numeric_limits<double>::infinity() }; CHECK(hs_place_db_add(db, 1, w, v, 2, &slot) == HS_ERR_INVALID); }
    { const int32_t w[2] = { 5, 6 }; const double v[2] = { std::nan(""), .5 }; CHECK(hs_place_db_add(db, 1, w, v, 2, &slot) == HS_ERR_INVALID); }
    int32_t live = -1, slots = -1;
    CHECK(hs_place_db_size(db, &live, &slots) == HS_OK && live == 0 && slots == 0);
    // past the first slot capacity (1024) and the first pool capacity (65 536 entries): 1100 vectors of 64 entries = 70 400
    const int N = 1100, M = 64;
    for (int i = 0; i < N; i++) {
        CHECK(place_add(db, 1000 + 7919ull * (uint64_t)((i * 37) % N), M, n_words, &slot) == HS_OK && slot == i);
        if (i == 5 || i == 1023 || i == 1024 || i == 1030) CHECK(place_queries(db, n_words, i + 1) == 0);           // before and after each regrow: the order is rebuilt
        if (i < 20) CHECK(place_add(db2, (uint64_t)i, 1 + i % 7, 100, &slot) == HS_OK && slot == i);                 // the second database grows beside it
    }
    CHECK(hs_place_db_size(db, &live, &slots) == HS_OK && live == N && slots == N);
    // tombstones: erase every third, twice is refused, out of range is refused; query after it
    for (int i = 0; i < N; i += 3) CHECK(hs_place_db_erase(db, i) == HS_OK);
    CHECK(hs_place_db_erase(db, 0) != HS_OK && hs_place_db_erase(db, N) != HS_OK && hs_place_db_erase(db, -1) != HS_OK);
    CHECK(hs_place_db_size(db, &live, &slots) == HS_OK && live == N - (N + 2) / 3 && slots == N);
    CHECK(place_queries(db, n_words, N) == 0);
    CHECK(place_add(db, 99, M, n_words, &slot) == HS_OK && slot == N);                          // a tombstone's slot is not reused
    CHECK(place_queries(db, n_words, N + 1) == 0 && place_queries(db2, 100, 20) == 0);
    // clear keeps the allocations; reuse from slot 0
    CHECK(hs_place_db_clear(db) == HS_OK && hs_place_db_size(db, &live, &slots) == HS_OK && live == 0 && slots == 0);
    CHECK(place_queries(db, n_words, 0) == 0);
    for (int i = 0; i < 40; i++) CHECK(place_add(db, 5000 - (uint64_t)i, rnd(1, 200), n_words, &slot) == HS_OK && slot == i);
    CHECK(place_queries(db, n_words, 40) == 0);
    hs_place_db_destroy(db); hs_place_db_destroy(db2); hs_place_db_destroy(nullptr);
    hs_orb_destroy(h);
    if (alone) CHECK(same_live(before));
    return 0;
}

// ---- `threads <seed>`: everything that is shared between threads, for ThreadSanitizer (it runs under ASan + UBSan as well).  Every section starts its
// threads behind a barrier of its own and gives each a bounded amount of work.
struct Gate {
    std::atomic<int> waiting{0}; const int n;
    explicit Gate(int n_) : n(n_) {}
    void arrive() { waiting++; while (waiting.load() < n) std::this_thread::yield(); }
};
static int threads_mode(uint64_t seed)
{
    const Live before = live_now();
    std::atomic<int> bad{0};
    {   // hs_comm_available: its first call, from four threads at once (the dlopen of librccl happens once)
        Gate g(4); std::vector<std::thread> th; std::atomic<int> sum{0};
        for (int t = 0; t < 4; t++) th.emplace_back([&] { g.arrive(); sum += hs_comm_available(); (void)hs_comm_unavailable_reason(); });
        for (auto& t : th) t.join();
        CHECK(sum.load() == 0 || sum.load() == 4);
    }
    {   // the four sweeps at once: a handle (or two) per thread, a generator per thread
        Gate g(4); std::vector<std::thread> th;
        for (int t = 0; t < 4; t++) th.emplace_back([&, t] { rng.seed(seed * 100 + t); g.arrive(); if ((t & 1 ? map_sweep(4, false) : staged_sweep(4, false)) != 0) bad++; if ((t & 1 ? staged_sweep(3, false) : map_sweep(3, false)) != 0) bad++; });
        for (auto& t : th) t.join();
        CHECK(bad.load() == 0);
    }
    {   // handle churn on two threads while two others extract and match
        Gate g(4); std::vector<std::thread> th;
        for (int t = 0; t < 2; t++) th.emplace_back([&, t] {
            rng.seed(seed * 100 + 10 + t); g.arrive();
            for (int i = 0; i < 150; i++) { hs_orb_params p; hs_orb_default_params(&p); p.nfeatures = 100 + 50 * (i % 5); hs_orb* x = nullptr; if (hs_orb_create(&p, 0, &x) != HS_OK) { bad++; break; } if (i % 3 == 0 && hs_orb_reserve(x, 160 + i, 120, 1) != HS_OK) bad++; hs_orb_destroy(x); }
        });
        for (int t = 0; t < 2; t++) th.emplace_back([&, t] {
            rng.seed(seed * 100 + 20 + t); g.arrive();
            hs_orb_params p; hs_orb_default_params(&p); p.nfeatures = 300; hs_orb* x = nullptr;
            if (hs_orb_create(&p, 0, &x) != HS_OK || hs_orb_reserve(x, 320, 240, 1) != HS_OK) { bad++; return; }
            const int cap = hs_orb_max_keypoints(x); const std::vector<uint8_t> img = rand_bytes(320 * 240);
            std::vector<hs_keypoint> k(cap); std::vector<uint8_t> d((size_t)cap * 32); int32_t n = 0;
            for (int i = 0; i < 40; i++) {
                if (hs_orb_extract(x, img.data(), 320, 240, 320, k.data(), d.data(), cap, &n) != HS_OK) bad++;
                const int nq = rnd(1, 200), nt = rnd(1, 200); const std::vector<uint8_t> q = rand_bytes((size_t)nq * 32), tt = rand_bytes((size_t)nt * 32); std::vector<int32_t> bi(nq), bd(nq), sd(nq);
                if (hs_hamming_knn2(x, q.data(), nq, tt.data(), nt, bi.data(), bd.data(), sd.data()) != HS_OK) bad++;
            }
            hs_orb_destroy(x);
        });
        for (auto& t : th) t.join();
        CHECK(bad.load() == 0);
    }
    {   // place databases: one used from two threads under a mutex (the adaptor's discipline, HipPlaceRecognizer::mutex), one freely on a third
        hs_orb_params p; hs_orb_default_params(&p); hs_orb *h1 = nullptr, *h2 = nullptr;
        CHECK(hs_orb_create(&p, 0, &h1) == HS_OK && hs_orb_create(&p, 0, &h2) == HS_OK);
        hs_place_db* shared = nullptr;
        CHECK(hs_place_db_create(h1, 2000, 0, &shared) == HS_OK);
        std::mutex mu; int added = 0;
        Gate g(3); std::vector<std::thread> th;
        th.emplace_back([&] { rng.seed(seed * 100 + 30); g.arrive(); for (int i = 0; i < 300; i++) { std::lock_guard<std::mutex> l(mu); int32_t s = -1; if (place_add(shared, 10 + (uint64_t)i, rnd(1, 60), 2000, &s) != HS_OK || s != added) bad++; added++; if (i % 50 == 49 && hs_place_db_erase(shared, s) != HS_OK) bad++; } });
        th.emplace_back([&] { rng.seed(seed * 100 + 31); g.arrive(); for (int i = 0; i < 120; i++) { std::lock_guard<std::mutex> l(mu); if (place_queries(shared, 2000, added) != 0) bad++; } });
        th.emplace_back([&] {
            rng.seed(seed * 100 + 32); g.arrive();
            hs_place_db* own = nullptr;
            if (hs_place_db_create(h2, 500, 0, &own) != HS_OK) { bad++; return; }
            for (int i = 0; i < 200; i++) { int32_t s = -1; if (place_add(own, (uint64_t)i, rnd(1, 40), 500, &s) != HS_OK) bad++; if (i % 20 == 19 && place_queries(own, 500, i + 1) != 0) bad++; }
            hs_place_db_destroy(own);
        });
        for (auto& t : th) t.join();
        hs_place_db_destroy(shared); hs_orb_destroy(h1); hs_orb_destroy(h2);
        CHECK(bad.load() == 0);
    }
    {   // the vocabulary loaders on good and corrupted files, four threads; hs_vocab_last_error is the calling thread's own
        char dir[] = "/tmp/hs_host_sanitize_XXXXXX";
        CHECK(mkdtemp(dir) != nullptr);
        const std::string good = std::string(dir) + "/v.bin", gtxt = std::string(dir) + "/v.txt";
        std::vector<int32_t> cb, cc, word; std::vector<uint8_t> desc; std::vector<float> weight;
        hs_vocab* v = make_vocab(4, 3, cb, cc, desc, word, weight);
        CHECK(v != nullptr && hs_vocab_save(v, good.c_str()) == HS_OK && hs_vocab_save(v, gtxt.c_str()) == HS_OK);
        hs_vocab_destroy(v);
        const std::vector<uint8_t> bytes = slurp(good);
        Gate g(4); std::vector<std::thread> th;
        for (int t = 0; t < 4; t++) th.emplace_back([&, t] {
            rng.seed(seed * 100 + 40 + t); g.arrive();
            const std::string mine = std::string(dir) + "/bad" + std::to_string(t) + ".bin";
            for (int i = 0; i < 40; i++) {
                hs_vocab* a = nullptr;
                if (t & 1) {                                         // the odd threads only ever load good files: their error text must stay empty
                    if (hs_vocab_load(i & 1 ? good.c_str() : gtxt.c_str(), &a) != HS_OK || !a || hs_vocab_last_error()[0] != 0) bad++;
                } else {
                    std::vector<uint8_t> b = bytes; b.resize((size_t)rnd(0, (int)b.size() - 1));
                    spit(mine, b);
                    if (hs_vocab_load(mine.c_str(), &a) == HS_OK ? a == nullptr : (a != nullptr || hs_vocab_last_error()[0] == 0)) bad++;
                }
                if (a) hs_vocab_destroy(a);
            }
            unlink(mine.c_str());
        });
        for (auto& t : th) t.join();
        unlink(good.c_str()); unlink(gtxt.c_str()); rmdir(dir);
        CHECK(bad.load() == 0);
    }
    CHECK(hs_frame_cache_clear(0) == HS_OK);
    CHECK(same_live(before));
    return 0;
}

// exactly one of hs_orb_destroy and the last borrower's release frees the handle
static int borrow_race()
{
    // ---- a handle outliving its communicators: hs_orb_destroy and the last borrower's release race on two threads; exactly one of them frees
    // the handle (ASan: a double free or a leak fails the run), in either order and with several borrowers
    for (int i = 0; i < 200; i++) {
        hs_orb_params p; hs_orb_default_params(&p);
        hs_orb* ex = nullptr;
        CHECK(hs_orb_create(&p, 0, &ex) == HS_OK);
        const int nb = 1 + i % 3;
        for (int b = 0; b < nb; b++) hs_orb_borrow(ex, +1);
        CHECK(hs_orb_borrowers(ex) == nb);
        std::atomic<int> go{0};
        std::thread td([&] { while (!go.load()) {} hs_orb_destroy(ex); });
        std::thread tb([&] { while (!go.load()) {} for (int b = 0; b < nb; b++) hs_orb_borrow(ex, -1); });
        go.store(1);
        td.join(); tb.join();
    }

    return 0;
}

static int frame_cache_section(uint64_t seed)
{
    // ---- the frame cache (hs_frame_*): publish after an extraction, find by keypoints, the *_frame(s) entry points, release, slot reuse after 16
    //      publishes, refusals (no extraction to publish, unknown tokens, a count that disagrees); then publishers, finders and consumers on four threads
    {
        hs_orb_params p; hs_orb_default_params(&p); p.nfeatures = 300;
        hs_orb *ex = nullptr, *mh = nullptr;
        CHECK(hs_orb_create(&p, 0, &ex) == HS_OK && hs_orb_create(&p, 0, &mh) == HS_OK);
        const int w = 320, h = 240;
        std::vector<uint8_t> img((size_t)w * h);
        for (auto& v : img) v = (uint8_t)rng();
        CHECK(hs_orb_reserve(ex, w, h, 1) == HS_OK);
        const int cap = hs_orb_max_keypoints(ex);
        std::vector<hs_keypoint> k(cap); std::vector<uint8_t> d((size_t)cap * 32); int32_t n = 0;
        hs_frame_token tok = 0;
        CHECK(hs_frame_publish(ex, 0, k.data(), 10, &tok) != HS_OK && tok == 0);                 // nothing extracted yet
        CHECK(hs_orb_extract(ex, img.data(), w, h, w, k.data(), d.data(), cap, &n) == HS_OK);
        // (the stub runs no kernels: fabricate a result of 40 keypoints to publish)
        const int nk = 40;
        for (int i = 0; i < nk; i++) k[i] = hs_keypoint{ 20.f + i, 30.f + 2 * i, 31.f, (float)i, 50.f, 0 };
        CHECK(hs_frame_publish(ex, 1, k.data(), nk, &tok) != HS_OK);                              // image index beyond the call's batch
        CHECK(hs_frame_publish(ex, 0, k.data(), cap + 1, &tok) != HS_OK);                         // more keypoints than the call could have produced
        CHECK(hs_frame_publish(ex, 0, k.data(), nk, &tok) == HS_OK && tok != 0);
        int32_t ninfo = 0; hs_frame_token found = 0;
        CHECK(hs_frame_info(0, tok, &ninfo) == HS_OK && ninfo == nk);
        CHECK(hs_frame_find(0, k.data(), nk, &found) == HS_OK && found == tok);
        CHECK(hs_frame_find(0, k.data(), nk - 1, &found) != HS_OK && found == 0);
        CHECK(hs_frame_find(1, k.data(), nk, &found) != HS_OK);                                    // another device's cache
        { std::vector<hs_keypoint> k2(k.begin(), k.begin() + nk); k2[7].response += 1.f; CHECK(hs_frame_find(0, k2.data(), nk, &found) != HS_OK); }
        hs_frame_view F; memset(&F, 0, sizeof(F));
        F.fx = F.fy = 300.f; F.cx = 160.f; F.cy = 120.f; F.max_x = (float)w; F.max_y = (float)h; F.size_ref = 31.f; F.n = nk; F.Rcw[0] = F.Rcw[4] = F.Rcw[8] = 1.f;
        std::vector<hs_landmark> lm(25); memset(lm.data(), 0, lm.size() * sizeof(hs_landmark));
        for (size_t i = 0; i < lm.size(); i++) { lm[i].pos[2] = 5.f; lm[i].size = 0.5f; lm[i].max_dist = 100.f; lm[i].assoc_kp = -1; }
        hs_proj_params pp; memset(&pp, 0, sizeof(pp)); pp.th = 3.f; pp.score_threshold = 100.f; pp.second_best_ratio = 0.8f; pp.frac_smaller = 0.5f; pp.frac_larger = 1.5f;
        std::vector<int32_t> mi(lm.size()); std::vector<float> md(lm.size()); int32_t nm = -1;
        CHECK(hs_search_by_projection_frame(mh, tok, &F, lm.data(), (int)lm.size(), &pp, mi.data(), md.data(), &nm) == HS_OK);
        F.n = nk - 1;
        CHECK(hs_search_by_projection_frame(mh, tok, &F, lm.data(), (int)lm.size(), &pp, mi.data(), md.data(), &nm) != HS_OK);      // count disagrees with the published frame
        F.n = nk;
        CHECK(hs_search_by_projection_frame(mh, tok + 1000, &F, lm.data(), (int)lm.size(), &pp, mi.data(), md.data(), &nm) != HS_OK);
        hs_stereo_params sp{ 300.f, 36.f, h, 100.f, 50.f, 31.f };
        std::vector<float> ur(nk), dz(nk);
        CHECK(hs_stereo_match_frames(mh, tok, tok, &sp, ur.data(), dz.data()) == HS_OK);
        CHECK(hs_stereo_match_frames(mh, tok, 0, &sp, ur.data(), dz.data()) != HS_OK);
        CHECK(hs_frame_release(0, tok) == HS_OK && hs_frame_release(0, tok) != HS_OK && hs_frame_info(0, tok, &ninfo) != HS_OK);
        // slot reuse: 17 more publishes of frames of different sizes (the slots' buffers grow) push the oldest out
        CHECK(hs_frame_publish(ex, 0, k.data(), nk, &tok) == HS_OK);
        for (int r = 0; r < 17; r++) { hs_frame_token t2 = 0; k[0].x = 500.f + r; CHECK(hs_frame_publish(ex, 0, k.data(), 1 + (r * 37) % cap, &t2) == HS_OK && t2 > tok); }
        CHECK(hs_frame_info(0, tok, &ninfo) != HS_OK);
        // four threads: two extractors publishing, one finder, one consumer (ASan: a slot freed or refilled under a reader fails the run)
        hs_orb* ex2 = nullptr;
        CHECK(hs_orb_create(&p, 0, &ex2) == HS_OK && hs_orb_reserve(ex2, w, h, 1) == HS_OK);
        std::vector<hs_keypoint> kb(cap); std::vector<uint8_t> db((size_t)cap * 32); int32_t nb2 = 0;
        CHECK(hs_orb_extract(ex2, img.data(), w, h, w, kb.data(), db.data(), cap, &nb2) == HS_OK);
        std::atomic<int> stop{0}, bad{0}; std::atomic<uint64_t> latest{0};
        auto publisher = [&](hs_orb* hx, int salt) {
            std::vector<hs_keypoint> kk(nk);
            for (int it = 0; it < 400; it++) {
                for (int i = 0; i < nk; i++) kk[i] = hs_keypoint{ (float)(salt + it), (float)i, 31.f, 0.f, 1.f, 0 };
                hs_frame_token t = 0;
                const int st = hs_frame_publish(hx, 0, kk.data(), 1 + (it * 7 + salt) % nk, &t);
                if (st == HS_OK) latest.store(t); else if (st != HS_ERR_CAPACITY) bad++;
            }
        };
        std::thread t1(publisher, ex, 1000), t2(publisher, ex2, 5000);
        std::thread t3([&] { std::mt19937_64 rng(seed + 3) /* its own: the main generator stays what the seed made it */; std::vector<hs_keypoint> kk(nk); while (!stop.load()) { for (int i = 0; i < nk; i++) kk[i] = hs_keypoint{ 1000.f + (float)(rng() % 400), (float)i, 31.f, 0.f, 1.f, 0 }; hs_frame_token t = 0; (void)hs_frame_find(0, kk.data(), 1 + (int)(rng() % nk), &t); } });
        std::thread t4([&] {
            hs_frame_view G = F; std::vector<int32_t> mi2(lm.size()); std::vector<float> md2(lm.size()); int32_t nm2 = 0;
            while (!stop.load()) {
                const hs_frame_token t = latest.load(); int32_t cnt = 0;
                if (t && hs_frame_info(0, t, &cnt) == HS_OK) { G.n = cnt; const int st = hs_search_by_projection_frame(mh, t, &G, lm.data(), (int)lm.size(), &pp, mi2.data(), md2.data(), &nm2); if (st != HS_OK && st != HS_ERR_INVALID) bad++; }
            }
        });
        t1.join(); t2.join(); stop.store(1); t3.join(); t4.join();
        CHECK(bad.load() == 0);
        hs_orb_destroy(ex); hs_orb_destroy(ex2); hs_orb_destroy(mh);
        CHECK(hs_frame_cache_clear(0) == HS_OK && hs_frame_cache_clear(0) == HS_OK && hs_frame_cache_clear(3) == HS_OK);      // (LeakSanitizer: nothing of the cache may outlive this)
        CHECK(hs_frame_info(0, latest.load(), &ninfo) != HS_OK);
    }

    return 0;
}

// ---- `host_sanitize refusals`: a refused call enqueues nothing.  Every enqueue-only `_device` entry point that is a stage of a resident chain, and
// every chain, gets one valid argument set at small sizes (no kernel runs under the stub) and then one knock-out at a time: every pointer argument and
// every pointer field of every struct argument NULL (found by scanning the argument set for words that point into the arena every buffer comes from),
// every struct argument NULL, every integer at its first refused value, the 16-byte aligned arrays off their alignment, sensor != 0 without uR, the
// frame_result alias.  Each call returns HS_OK or HS_ERR_INVALID; across a refused call no counter of the stub moves (launches, their digest, copies,
// memsets, allocations); an accepted call launches what the valid call launches (an integer knock-out may leave it less); the knock-outs a chain's LATER stages refuse (MUST below) are refused by the chain.
namespace refusals {
struct Arena {
    std::vector<uint8_t> mem = std::vector<uint8_t>(4u << 20, 0); size_t used = 0;
    template <class T> T* take(size_t n) { used = (used + 255) & ~(size_t)255; T* p = reinterpret_cast<T*>(mem.data() + used); used += std::max<size_t>(n * sizeof(T), 16); return p; }
    bool holds(const void* p) const { return (const uint8_t*)p >= mem.data() && (const uint8_t*)p < mem.data() + mem.size(); }
};
struct Args {                                                     // plain data: a knock-out edits a copy
    hs_frame_view F; hs_kf_table T; hs_kf_features K; hs_track_state S; hs_track_out O; hs_track_initial_out IO; hs_keyframe_out KO;
    hs_track_params tp; hs_track_refkf_params rp; hs_keyframe_params kp; hs_proj_params pp;
    int has_F, has_T, has_K, has_S, has_O, has_IO, has_KO, has_tp, has_rp, has_kp, has_pp;      // 0: the call gets NULL for the struct
    const hs_vocab_dev* vocab;
    float *Tpred, *Tlast, *Tentry, *Tcw, *depth; hs_keypoint* last_kps; int32_t *last_lm, *neigh, *parent, *kf_slot, *ref_slot, *counts; int64_t* q_off;
    hs_landmark* lms; hs_track_result* track_result; void* work;
    int n_last, neigh_cap, cap, kf_cap, new_cap;
};
struct Knock { std::string name; std::function<void(Args&)> apply; bool size = false; /* an integer: an accepted call may find nothing to launch */ };
struct Entry { const char* name; std::function<int(hs_orb*, const Args&)> call; std::vector<std::string> must; };
#define P(x) (a.has_##x ? &a.x : nullptr)

static int run(bool list /*print every call's status: two commits that refuse the same calls print the same lines*/)
{
    hs_orb_params p; hs_orb_default_params(&p); p.nfeatures = 300;
    hs_orb* h = nullptr;
    CHECK(hs_orb_create(&p, 0, &h) == HS_OK);
    const int n = 100, n_last = 80, L = 120, n_kf = 5, cap = 60, kf_cap = 8, new_cap = 16, neigh_cap = 10, n_kps_kf = 12;
    Arena ar;
    Args v; memset(&v, 0, sizeof(v));
    v.has_F = v.has_T = v.has_K = v.has_S = v.has_O = v.has_IO = v.has_KO = v.has_tp = v.has_rp = v.has_kp = v.has_pp = 1;
    v.n_last = n_last; v.neigh_cap = neigh_cap; v.cap = cap; v.kf_cap = kf_cap; v.new_cap = new_cap;
    v.F.fx = v.F.fy = 300.f; v.F.cx = 160.f; v.F.cy = 120.f; v.F.max_x = 320.f; v.F.max_y = 240.f; v.F.size_ref = 31.f; v.F.mbf = 40.f; v.F.sensor = 1; v.F.n = n;
    v.F.kps = ar.take<hs_keypoint>(n); v.F.desc = ar.take<uint8_t>((size_t)n * 32); v.F.uR = ar.take<float>(n); v.F.kp_lm_obs = ar.take<int32_t>(n);
    v.T = hs_kf_table{ L, n_kf, ar.take<int64_t>(L + 1), ar.take<int32_t>(16), ar.take<int32_t>(16), ar.take<uint8_t>(L), ar.take<int32_t>(L), ar.take<uint8_t>(n_kf), ar.take<int64_t>(n_kf) };
    v.K = hs_kf_features{ n_kf, ar.take<int64_t>(n_kf + 1), ar.take<hs_keypoint>(n_kps_kf), ar.take<uint8_t>(n_kps_kf * 32), ar.take<int32_t>(n_kps_kf), ar.take<int32_t>(n_kps_kf), ar.take<float>(n_kps_kf) };
    v.S = hs_track_state{ ar.take<int32_t>(n), ar.take<uint8_t>(n), ar.take<int32_t>(1), ar.take<int32_t>(n) };
    const hs_local_map_out lo{ ar.take<int32_t>(n_kf), ar.take<int32_t>(1), ar.take<int32_t>(1), ar.take<uint8_t>(n_kf), ar.take<int32_t>(1), ar.take<uint8_t>(n), ar.take<int32_t>(cap), ar.take<int32_t>(1),
                               ar.take<hs_landmark>(cap), ar.take<int32_t>(cap), ar.take<float>(cap), ar.take<int32_t>(1) };
    v.O = hs_track_out{ ar.take<hs_pose_view>(2), ar.take<hs_pose_problem>(2), ar.take<hs_landmark>(n_last), ar.take<int32_t>(n_last), ar.take<float>(n_last), ar.take<int32_t>(1), ar.take<int32_t>(n_last),
                        ar.take<float>(n_last), ar.take<int32_t>(1), ar.take<int32_t>(n_last), ar.take<hs_pose_edge>(n), ar.take<uint8_t>(n), ar.take<int32_t>(2), ar.take<hs_pose_result>(1), lo,
                        ar.take<hs_pose_edge>(n), ar.take<uint8_t>(n), ar.take<int32_t>(1), ar.take<hs_pose_result>(1), ar.take<hs_track_result>(1) };
    v.IO = hs_track_initial_out{ ar.take<int32_t>(n), ar.take<float>(n), ar.take<int32_t>(n), ar.take<int32_t>(kf_cap), ar.take<int32_t>(n), ar.take<int32_t>(n), ar.take<hs_pose_view>(1),
                                 ar.take<hs_pose_problem>(1), ar.take<hs_pose_edge>(n), ar.take<uint8_t>(n), ar.take<int32_t>(2), ar.take<hs_pose_result>(1), ar.take<float>(16),
                                 ar.take<hs_track_initial_result>(1), ar.take<hs_track_result>(1) };
    v.KO = hs_keyframe_out{ ar.take<hs_keyframe_result>(1), ar.take<hs_pose_view>(1), ar.take<int32_t>(new_cap), ar.take<float>(new_cap * 3), ar.take<hs_lm_entry_in>(new_cap), ar.take<hs_lm_obs>(new_cap),
                            ar.take<int64_t>(new_cap + 1), ar.take<int64_t>(new_cap + 1), ar.take<uint8_t>(new_cap * 32), ar.take<int32_t>(new_cap), ar.take<hs_landmark>(L + new_cap), L + new_cap };
    v.tp.th_motion = 7.f; v.tp.th_motion_wide = 14.f; v.tp.n_min_matches = 20; v.tp.th_local = 3.f; v.tp.nnratio_motion = 0.9f; v.tp.nnratio_local = 0.8f; v.tp.th_high = 100.f; v.tp.sigma_ref = 1.f;
    v.tp.n_max_local_keyframes = 80; v.tp.n_neighbor_keyframes = 10;
    v.rp = hs_track_refkf_params{ 50.f, 0.7f, 15, 10 };
    v.kp.frame_id = 100; v.kp.last_keyframe_id = 10; v.kp.max_KF_interval = 30; v.kp.th_depth = 40.f; v.kp.n_min_points = 100; v.kp.ok_override = -1;
    v.pp.th = 3.f; v.pp.score_threshold = 100.f; v.pp.second_best_ratio = 0.8f; v.pp.frac_smaller = 0.5f; v.pp.frac_larger = 1.5f; v.pp.use_stereo = 1;
    v.Tpred = ar.take<float>(16); v.Tlast = ar.take<float>(16); v.Tentry = ar.take<float>(16); v.Tcw = ar.take<float>(16); v.depth = ar.take<float>(n);
    v.last_kps = ar.take<hs_keypoint>(n_last); v.last_lm = ar.take<int32_t>(n_last); v.neigh = ar.take<int32_t>(n_kf * neigh_cap); v.parent = ar.take<int32_t>(n_kf);
    v.kf_slot = ar.take<int32_t>(1); v.ref_slot = ar.take<int32_t>(1); v.counts = ar.take<int32_t>(1); v.q_off = ar.take<int64_t>(2); v.lms = ar.take<hs_landmark>(L);
    v.track_result = ar.take<hs_track_result>(1);
    v.work = ar.take<uint8_t>(std::max(hs_track_initial_work_bytes(n, n_last, L, cap, kf_cap), hs_keyframe_work_bytes(n, kf_cap, new_cap)));
    std::vector<int32_t> cb, cc, word; std::vector<uint8_t> vdesc; std::vector<float> weight;
    { hs_vocab* voc = make_vocab(3, 3, cb, cc, vdesc, word, weight); CHECK(voc != nullptr); hs_vocab_destroy(voc); }
    const hs_vocab_tree tree{ (int32_t)cb.size(), 3, cb.data(), cc.data(), vdesc.data(), word.data(), weight.data(), nullptr };
    hs_vocab_dev* vocab = nullptr;
    CHECK(hs_vocab_upload(h, &tree, 1, &vocab) == HS_OK && vocab);
    v.vocab = vocab;
    CHECK(ar.used < ar.mem.size());

    // ---- the knock-outs
    std::vector<Knock> kos;
    static const struct { size_t off; const char* name; } parts[] = {
        { offsetof(Args, F), "F" }, { offsetof(Args, T), "T" }, { offsetof(Args, K), "K" }, { offsetof(Args, S), "st" }, { offsetof(Args, O), "out" }, { offsetof(Args, IO), "iout" },
        { offsetof(Args, KO), "kout" }, { offsetof(Args, tp), "params" }, { offsetof(Args, vocab), "argument" } };
    for (size_t off = 0; off + sizeof(void*) <= sizeof(Args); off += sizeof(void*)) {
        void* word_at; memcpy(&word_at, (const char*)&v + off, sizeof(void*));
        if (!ar.holds(word_at)) continue;
        size_t k = 0;
        while (k + 1 < sizeof(parts) / sizeof(parts[0]) && parts[k + 1].off <= off) k++;
        kos.push_back({ std::string(parts[k].name) + " + " + std::to_string(off - parts[k].off) + " = NULL", [off](Args& a) { memset((char*)&a + off, 0, sizeof(void*)); } });
    }
    const size_t n_scanned = kos.size();
    CHECK(n_scanned == 4 + 7 + 6 + 4 + (19 + 12) + 15 + 11 + 16);      // every pointer field of the seven structs and the sixteen pointer arguments were found
    kos.push_back({ "F->uR = NULL, sensor 1", [](Args& a) { a.F.uR = nullptr; } });
    kos.push_back({ "out->local.weights = NULL", [](Args& a) { a.O.local.weights = nullptr; } });
    kos.push_back({ "out->local.match_idx = NULL", [](Args& a) { a.O.local.match_idx = nullptr; } });
    kos.push_back({ "d_parent = NULL", [](Args& a) { a.parent = nullptr; } });
    kos.push_back({ "d_neigh = NULL", [](Args& a) { a.neigh = nullptr; } });
    kos.push_back({ "T->lm_obs_offsets = NULL", [](Args& a) { a.T.lm_obs_offsets = nullptr; } });
    kos.push_back({ "T->kf_bad = NULL", [](Args& a) { a.T.kf_bad = nullptr; } });
    kos.push_back({ "cap = 0", [](Args& a) { a.cap = 0; }, true });
    kos.push_back({ "vocab = NULL", [](Args& a) { a.vocab = nullptr; } });
    kos.push_back({ "F = NULL", [](Args& a) { a.has_F = 0; } }); kos.push_back({ "T = NULL", [](Args& a) { a.has_T = 0; } }); kos.push_back({ "K = NULL", [](Args& a) { a.has_K = 0; } });
    kos.push_back({ "st = NULL", [](Args& a) { a.has_S = 0; } }); kos.push_back({ "out = NULL", [](Args& a) { a.has_O = 0; } }); kos.push_back({ "iout = NULL", [](Args& a) { a.has_IO = 0; } });
    kos.push_back({ "kout = NULL", [](Args& a) { a.has_KO = 0; } }); kos.push_back({ "tp = NULL", [](Args& a) { a.has_tp = 0; } }); kos.push_back({ "rp = NULL", [](Args& a) { a.has_rp = 0; } });
    kos.push_back({ "prm = NULL", [](Args& a) { a.has_kp = 0; } }); kos.push_back({ "pp = NULL", [](Args& a) { a.has_pp = 0; } });
    kos.push_back({ "n = 0", [](Args& a) { a.F.n = 0; }, true }); kos.push_back({ "n = 65536", [](Args& a) { a.F.n = 65536; }, true }); kos.push_back({ "L = 0", [](Args& a) { a.T.L = 0; }, true });
    kos.push_back({ "kf_cap = 0", [](Args& a) { a.kf_cap = 0; }, true }); kos.push_back({ "n_last = 0", [](Args& a) { a.n_last = 0; }, true }); kos.push_back({ "new_cap = -1", [](Args& a) { a.new_cap = -1; }, true });
    kos.push_back({ "neigh_cap = -1", [](Args& a) { a.neigh_cap = -1; }, true });
    kos.push_back({ "d_lms + 4", [](Args& a) { a.lms = (hs_landmark*)((char*)a.lms + 4); } });
    kos.push_back({ "out->last_lms + 4", [](Args& a) { a.O.last_lms = (hs_landmark*)((char*)a.O.last_lms + 4); } });
    kos.push_back({ "out->local.lms + 4", [](Args& a) { a.O.local.lms = (hs_landmark*)((char*)a.O.local.lms + 4); } });
    kos.push_back({ "out->edges_motion + 8", [](Args& a) { a.O.edges_motion = (hs_pose_edge*)((char*)a.O.edges_motion + 8); } });
    kos.push_back({ "out->edges_local + 8", [](Args& a) { a.O.edges_local = (hs_pose_edge*)((char*)a.O.edges_local + 8); } });
    kos.push_back({ "iout->edges + 8", [](Args& a) { a.IO.edges = (hs_pose_edge*)((char*)a.IO.edges + 8); } });
    kos.push_back({ "iout->frame_result = out->result", [](Args& a) { a.IO.frame_result = a.O.result; } });

    // ---- the entry points.  MUST: what only a later stage of the chain reads, so that the chain has to ask that stage's predicate before its first launch
    const std::vector<std::string> uR{ "F->uR = NULL, sensor 1" };
    std::vector<std::string> local{ "out->local.weights = NULL", "out->local.match_idx = NULL", "d_parent = NULL", "d_neigh = NULL", "T->lm_obs_offsets = NULL", "T->kf_bad = NULL", "cap = 0" };
    local.push_back(uR[0]);
    auto motion_model = [](hs_orb* h, const Args& a) { return hs_track_motion_model_device(h, P(F), a.Tpred, a.last_kps, a.last_lm, a.n_last, P(T), a.lms, P(tp), P(S), P(O), a.work, nullptr); };
    auto local_map = [](hs_orb* h, const Args& a) { return hs_track_local_map_device(h, P(F), a.Tcw, P(T), a.lms, a.neigh, a.neigh_cap, a.parent, a.cap, P(tp), P(S), P(O), a.work, nullptr); };
    auto initial = [](int vv) { return [vv](hs_orb* h, const Args& a) {
        return hs_track_initial_device(h, P(F), vv, a.Tpred, a.last_kps, a.last_lm, a.n_last, a.vocab, P(K), a.kf_slot, a.kf_cap, a.Tlast, a.Tentry, P(T), a.lms, P(tp), P(rp), P(S), P(O), P(IO), a.work, nullptr); }; };
    auto normal = [](int vv) { return [vv](hs_orb* h, const Args& a) {
        return hs_track_normal_device(h, P(F), vv, a.Tpred, a.last_kps, a.last_lm, a.n_last, a.vocab, P(K), a.kf_slot, a.kf_cap, a.Tlast, a.Tentry, P(T), a.lms, a.neigh, a.neigh_cap, a.parent, a.cap, P(tp),
                                      P(rp), P(S), P(O), P(IO), a.work, nullptr); }; };
    auto map_search = [](bool posed) { return [posed](hs_orb* h, const Args& a) {
        const hs_local_map_out* o = a.has_O ? &a.O.local : nullptr;
        return posed ? hs_local_map_search_posed_device(h, P(T), a.S.kp_lm, a.F.n, a.neigh, a.neigh_cap, a.parent, 80, 10, P(F), a.O.pose_view, a.lms, P(pp), a.cap, o, a.work, nullptr)
                     : hs_local_map_search_device(h, P(T), a.S.kp_lm, a.F.n, a.neigh, a.neigh_cap, a.parent, 80, 10, P(F), a.lms, P(pp), a.cap, o, a.work, nullptr); }; };
    auto projection = [](bool posed) { return [posed](hs_orb* h, const Args& a) {
        const hs_local_map_out& o = a.O.local;
        return posed ? hs_search_by_projection_posed_device(h, P(F), a.O.pose_view, o.lms, a.cap, P(pp), o.match_idx, o.match_dist, o.n_matches, nullptr)
                     : hs_search_by_projection_device(h, P(F), o.lms, a.cap, P(pp), o.match_idx, o.match_dist, o.n_matches, nullptr); }; };
    const std::vector<Entry> entries = {
        { "hs_pose_views_device", [](hs_orb* h, const Args& a) { return hs_pose_views_device(h, a.Tpred, a.O.pose_view, nullptr); }, {} },
        { "hs_frame_associate_device", [](hs_orb* h, const Args& a) { return hs_frame_associate_device(h, a.F.n, a.T.L, a.S.kp_lm, a.S.kp_outl, a.S.n_matches, a.n_last, a.O.op_view, a.last_lm, a.work, nullptr); }, {} },
        { "hs_frame_views_device", [](hs_orb* h, const Args& a) { return hs_frame_views_device(h, a.F.n, a.S.kp_lm, a.S.kp_outl, a.S.n_matches, P(T), 1, a.S.kp_lm_obs, nullptr); }, {} },
        { "hs_track_discard_device", [](hs_orb* h, const Args& a) { return hs_track_discard_device(h, HS_TRACK_MOTION, a.O.edges_motion, a.O.n_edges_motion, a.F.n, a.O.outlier_motion, a.O.pose_motion, P(T), a.F.sensor,
                                                                                                   a.S.kp_lm, a.S.kp_outl, a.S.n_matches, a.counts, nullptr); }, {} },
        { "hs_track_motion_model_device", motion_model, uR },
        { "hs_track_local_map_device", local_map, local },
        { "hs_track_frame_device", [](hs_orb* h, const Args& a) { return hs_track_frame_device(h, P(F), a.Tpred, a.last_kps, a.last_lm, a.n_last, P(T), a.lms, a.neigh, a.neigh_cap, a.parent, a.cap, P(tp), P(S), P(O),
                                                                                               a.work, nullptr); }, local },
        { "hs_search_by_bow_kf_device", [](hs_orb* h, const Args& a) { return hs_search_by_bow_kf_device(h, P(K), a.kf_slot, P(T), a.F.kps, a.F.desc, a.IO.bow_node, a.IO.bow_weight, a.F.n, 50.f, 0.7f, a.IO.match_kf,
                                                                                                         a.kf_cap, a.IO.op_view, a.IO.op_lm, a.counts, nullptr, nullptr); }, {} },
        { "hs_frame_associate_views_device", [](hs_orb* h, const Args& a) { return hs_frame_associate_views_device(h, a.F.n, a.T.L, a.S.kp_lm, a.S.kp_outl, a.S.n_matches, a.IO.op_view, a.IO.op_lm, a.work, nullptr); }, {} },
        { "hs_track_reference_keyframe_device", [](hs_orb* h, const Args& a) { return hs_track_reference_keyframe_device(h, P(F), a.vocab, P(K), a.kf_slot, a.kf_cap, a.Tlast, a.Tentry, a.track_result, P(T), a.lms, P(tp),
                                                                                                                         P(rp), P(S), P(IO), a.work, nullptr); }, {} },
        { "hs_track_initial_device (valid velocity)", initial(1), uR },
        { "hs_track_initial_device (no velocity)", initial(0), {} },
        { "hs_track_normal_device (valid velocity)", normal(1), local },
        { "hs_track_normal_device (no velocity)", normal(0), local },
        { "hs_keyframe_reference_device", [](hs_orb* h, const Args& a) { return hs_keyframe_reference_device(h, a.F.n, P(S), P(T), a.ref_slot, a.KO.result, a.work, nullptr); }, {} },
        { "hs_keyframe_gate_device", [](hs_orb* h, const Args& a) { return hs_keyframe_gate_device(h, a.track_result, P(kp), a.KO.result, nullptr); }, {} },
        { "hs_keyframe_clean_device", [](hs_orb* h, const Args& a) { return hs_keyframe_clean_device(h, a.F.n, P(S), P(T), a.KO.result, nullptr); }, {} },
        { "hs_keyframe_need_device", [](hs_orb* h, const Args& a) { return hs_keyframe_need_device(h, a.F.n, a.F.sensor, a.depth, P(S), P(T), P(K), a.ref_slot, a.track_result, P(kp), a.KO.result, nullptr); }, {} },
        { "hs_keyframe_create_device", [](hs_orb* h, const Args& a) { return hs_keyframe_create_device(h, P(F), a.depth, a.Tcw, P(S), P(T), P(kp), a.new_cap, P(KO), a.work, nullptr); }, {} },
        { "hs_keyframe_discard_device", [](hs_orb* h, const Args& a) { return hs_keyframe_discard_device(h, a.F.n, P(S), a.KO.result, nullptr); }, {} },
        { "hs_track_keyframe_device", [](hs_orb* h, const Args& a) { return hs_track_keyframe_device(h, P(F), a.depth, a.Tcw, P(T), P(K), a.track_result, P(kp), P(S), a.ref_slot, a.new_cap, P(KO), a.work, nullptr); }, {} },
        { "hs_local_keyframes_device", [](hs_orb* h, const Args& a) { return hs_local_keyframes_device(h, a.T.n_kf, a.O.local.weights, a.T.kf_bad, a.neigh, a.neigh_cap, a.parent, 80, 10, a.O.local.local,
                                                                                                       a.O.local.n_local, nullptr); }, {} },
        { "hs_local_points_device", [](hs_orb* h, const Args& a) { return hs_local_points_device(h, P(T), a.O.local.local, a.S.kp_lm, a.F.n, a.O.local.frame_remove, a.O.local.sel, a.cap, a.O.local.n_sel, a.work, nullptr); }, {} },
        { "hs_landmark_gather_device", [](hs_orb* h, const Args& a) { return hs_landmark_gather_device(h, a.lms, a.T.L, a.O.local.sel, a.O.local.n_sel, a.cap, a.O.local.lms, nullptr); }, {} },
        { "hs_local_map_search_device", map_search(false), {} },
        { "hs_local_map_search_posed_device", map_search(true), {} },
        { "hs_pose_optimize_device", [](hs_orb* h, const Args& a) { return hs_pose_optimize_device(h, 1, a.O.problem, nullptr, a.O.n_edges_local, a.F.n, a.O.edges_local, a.O.outlier_local, a.O.pose_local, nullptr, nullptr); }, {} },
        { "hs_pose_edges_device", [](hs_orb* h, const Args& a) { return hs_pose_edges_device(h, P(F), a.lms, a.T.L, a.S.kp_lm, 1.f, a.O.edges_local, a.F.n, a.O.n_edges_local, nullptr, nullptr); }, {} },
        { "hs_kf_votes_device", [](hs_orb* h, const Args& a) { return hs_kf_votes_device(h, P(T), 1, a.q_off, a.S.kp_lm, nullptr, 1, 1, a.O.local.weights, a.O.local.max_slot, a.O.local.max_count, nullptr, nullptr, 0,
                                                                                         a.counts, nullptr); }, {} },
        { "hs_search_by_projection_device", projection(false), {} },
        { "hs_search_by_projection_posed_device", projection(true), {} },
        { "hs_bow_transform_device", [](hs_orb* h, const Args& a) { return hs_bow_transform_device(h, a.vocab, a.F.desc, nullptr, a.F.n, a.IO.bow_word, a.IO.bow_weight, a.IO.bow_node, nullptr); }, {} },
    };

    int failures = 0, total_refused = 0;
    auto counters_moved = [](const unsigned long long* c0) { unsigned long long c1[14]; hip_stub_counters(c1); return memcmp(c0, c1, sizeof(c1)) != 0; };
    for (const Entry& e : entries) {
        unsigned long long c0[14];
        hip_stub_counters(c0);
        const long l0 = hip_stub_launches();
        const int rc0 = e.call(h, v);
        const long valid_launches = hip_stub_launches() - l0;
        if (rc0 != HS_OK || valid_launches < 1) { printf("REFUSALS FAILED %s: the valid call returned %d (%s) after %ld launches\n", e.name, rc0, hs_orb_last_error(h), valid_launches); failures++; continue; }
        int refused = 0;
        for (const Knock& k : kos) {
            Args a = v;
            k.apply(a);
            hip_stub_counters(c0);
            const long l1 = hip_stub_launches();
            const int rc = e.call(h, a);
            const long launched = hip_stub_launches() - l1;
            const bool moved = counters_moved(c0), must = std::find(e.must.begin(), e.must.end(), k.name) != e.must.end();
            refused += rc == HS_ERR_INVALID;
            if (list) printf("status %d: %s, %s\n", rc, e.name, k.name.c_str());
            const char* what = rc != HS_OK && rc != HS_ERR_INVALID ? "a status that is neither HS_OK nor HS_ERR_INVALID" : rc == HS_ERR_INVALID && moved ? "refused after the stub's counters moved"
                             : rc == HS_OK && !k.size && launched != valid_launches ? "accepted, but not with the valid call's launches" : rc == HS_OK && must ? "accepted what a later stage refuses" : nullptr;
            if (what) { printf("REFUSALS FAILED %s, %s: %s (status %d, %ld launches enqueued)\n", e.name, k.name.c_str(), what, rc, launched); failures++; }
        }
        if (refused < 1) { printf("REFUSALS FAILED %s: no knock-out was refused\n", e.name); failures++; }
        printf("%-44s valid call: %3ld launches; %3d of %zu knock-outs refused\n", e.name, valid_launches, refused, kos.size());
        total_refused += refused;
    }
    hs_vocab_dev_destroy(vocab);
    hs_orb_destroy(h);
    if (failures) { printf("HOST SANITIZE REFUSALS FAILED: %d findings\n", failures); return 1; }
    printf("HOST SANITIZE REFUSALS OK: %zu entry points, %zu knock-outs each (%zu pointers found by the scan), %d calls refused, none of them moved a counter\n", entries.size(), kos.size(), n_scanned,
           total_refused);
    return 0;
}
#undef P
}  // namespace refusals

// ---- host_sanitize fastplan: hs_fast_launch_plan and hs_fast_overflow_bytes over a fixed table, under the knobs the environment sets (read through the
// knob table, as a handle reads them).  One line per tile width: a digest over every field of every launch record of the table and the overflow bytes
// of its geometry; then the narrow / wide choice.  tests/golden/fast_launch_digests.json holds the lines of the commit before the plan function existed.
namespace fastplan {
struct Fnv64 { uint64_t v = 0xcbf29ce484222325ull; void add(uint64_t x) { v ^= x; v *= 0x100000001b3ull; } };
static int run()
{
    const HsKnobs env = hs_read_knobs();
    static const int HCELL[] = { 32, 33, 34, 35, 38, 39, 48, 49, 64, 65, 96, 97, 125 }, BATCH[] = { 1, 2, 3, 8, 12, 32, 64, 128, 256 }, ITEMS[] = { 1, 7, 861, 1904 };
    for (int lc = 5; lc <= 6; lc++) {
        HsKnobs k = env; k.fast_cols = 4 << (lc - 2);           // 32 / 64: this tile width whatever the batch
        Fnv64 H; long n = 0;
        for (int hc : HCELL) for (int b : BATCH) for (int it : ITEMS) {
            const int n0 = it / 3;                                // the split's level-0 tail: the last third of the list
            const int range[3][3] = { { 0, it, 0 }, { 0, it - n0, 0 }, { it - n0, n0, 1 } };      // the whole list; head with spill slot 0; tail with slot 1
            for (int r = 0; r < (n0 > 0 ? 3 : 1); r++) {
                const HsFastLaunch P = hs_fast_launch_plan(k, hc, it, it, b, range[r][0], range[r][1], range[r][2]);
                CHECK(P.lc == lc && P.narrow == (lc == 5));
                const int64_t f[] = { P.lc, P.narrow, P.tr, P.lds.off_cnt, P.lds.pcap_max, P.lds.pcap_min, P.lds.total, P.nblk, P.ovf_stride, P.spill_base, P.item_first, P.items_per_img,
                                      P.total_work, P.force_scan_b, P.S.nq_log, P.S.mode, P.S.par, P.S.par_log, P.S.per_q, P.S.m_per_q, P.S.m_par, P.S.m_items };
                for (int64_t x : f) H.add((uint64_t)x);
                n++;
            }
            H.add((uint64_t)hs_fast_overflow_bytes(k, hc, it, it, b));
        }
        printf("fastplan lc %d: %ld launches, digest %016llx\n", lc, n, (unsigned long long)H.v);
    }
    Fnv64 H;
    for (int it : { 861, 1904 }) for (int b = 1; b <= 128; b++) H.add((uint64_t)hs_fast_narrow(env, it, b));
    printf("fastplan narrow: digest %016llx\n", (unsigned long long)H.v);
    return 0;
}
}  // namespace fastplan

// ---- host_sanitize fastsched: the work-unit schedule of k_fast_rows on the CPU.  The host half (hs_fast_launch_plan: mode, queue count, magic divisors)
// and the device half (hs_fast.h: fast_queue_size, unit_decode, fast_div — the very functions the kernel inlines) must together hand out every (item, image)
// of a launch exactly once.  Units are enumerated the way the kernel reaches them: per queue in modes 0-3, as [0, total_work) in the folded mode 4.
namespace fastsched {
static int check_div(const char* what, int a, int d, uint32_t m, int w)
{
    if (d >= 1 && fast_div(a, d, m) == a / d) return 0;
    printf("FAST SCHEDULE FAILED: unit %d: fast_div(%d, %d, %u) [%s] = %d, not %d\n", w, a, d, m, what, d >= 1 ? fast_div(a, d, m) : -1, d >= 1 ? a / d : -1);
    return 1;
}
static int launch(const HsKnobs& k, int lc, int batch, int items, long& units, long modes[5])
{
    HsKnobs kk = k; kk.fast_cols = 4 << (lc - 2);
    const HsFastLaunch P = hs_fast_launch_plan(kk, 31, items, items, batch, 0, items, 0);
    const FastSched& S = P.S;
    const int nq = 1 << S.nq_log;
    char where[160]; snprintf(where, sizeof(where), "batch %d, %d items, lc %d, nq knob %d, image_major %d, no_fold %d: mode %d, %d queues, %d workgroups", batch, items, lc, k.fast_nq, k.fast_image_major, k.fast_no_fold, S.mode, nq, P.nblk);
    if (P.total_work != items * batch || P.nblk < nq || P.nblk % nq != 0) { printf("FAST SCHEDULE FAILED: %s: the workgroups are no multiple of the queues\n", where); return 1; }
    if (S.mode < 0 || S.mode > 4) { printf("FAST SCHEDULE FAILED: %s: unknown mode\n", where); return 1; }
    std::vector<uint8_t> seen((size_t)P.total_work, 0);
    auto unit = [&](int w, int q, int idx) {
        // fast_div's operand pairs of this unit, restated from unit_decode
        int bad = 0;
        if (S.mode == 1 || S.mode == 2 || S.mode == 3) {
            bad += check_div("per_q", w, S.per_q, S.m_per_q, w);
            const int qq = S.per_q >= 1 ? w / S.per_q : 0, u = w - qq * S.per_q;
            if (S.mode == 1) bad += check_div("par", u, S.par, S.m_par, w);
            if (S.mode == 3) bad += check_div("par", (u << S.nq_log) + qq, S.par, S.m_par, w);
        } else if (S.mode == 4) bad += check_div("par", w, S.par, S.m_par, w);
        else bad += check_div("items", w, P.items_per_img, S.m_items, w);
        if (bad) { printf("  in %s (queue %d, index %d)\n", where, q, idx); return 1; }
        int img = -1;
        const int item = unit_decode(P.items_per_img, S, w, &img);
        const bool in_range = item >= 0 && item < items && img >= 0 && img < batch;
        if (!in_range || seen[(size_t)img * items + item]) {
            printf("FAST SCHEDULE FAILED: %s: unit %d (queue %d, index %d) decodes to item %d of image %d: %s\n", where, w, q, idx, item, img, in_range ? "handed out twice" : "out of range");
            return 1;
        }
        seen[(size_t)img * items + item] = 1;
        units++;
        return 0;
    };
    if (S.mode == 4) {
        if (P.total_work > 2 * P.nblk) { printf("FAST SCHEDULE FAILED: %s: a folded launch of more than two units per workgroup\n", where); return 1; }
        for (int w = 0; w < P.total_work; w++) if (unit(w, -1, w)) return 1;
    } else {
        for (int q = 0; q < nq; q++) {
            const int size = fast_queue_size(S, q, P.total_work, P.items_per_img);
            if (size > S.per_q) { printf("FAST SCHEDULE FAILED: %s: queue %d holds %d units, more than per_q = %d\n", where, q, size, S.per_q); return 1; }
            for (int idx = 0; idx < size; idx++) if (unit(q * S.per_q + idx, q, idx)) return 1;
        }
    }
    for (size_t i = 0; i < seen.size(); i++)
        if (!seen[i]) { printf("FAST SCHEDULE FAILED: %s: item %d of image %d is never handed out\n", where, (int)(i % items), (int)(i / items)); return 1; }
    modes[S.mode]++;
    return 0;
}
static int run()
{
    const HsKnobs env = hs_read_knobs();
    long units = 0, launches = 0, modes[5] = {};
    for (int nq : { 0, 8, 16 }) for (int variant = 0; variant < 3; variant++) {         // HS_FAST_NQ unset / 8 / 16, each plain, with HS_FAST_IMAGE_MAJOR and with HS_FAST_NO_FOLD
        HsKnobs k = env; k.fast_nq = nq; k.fast_image_major = variant == 1; k.fast_no_fold = variant == 2;
        for (int batch : { 1, 2, 3, 5, 8, 16, 24, 32, 33, 64 }) for (int items : { 1, 2, 7, 61 }) for (int lc = 5; lc <= 6; lc++) {
            if (launch(k, lc, batch, items, units, modes)) return 1;
            launches++;
        }
    }
    for (int m = 0; m < 5; m++) if (modes[m] == 0) { printf("FAST SCHEDULE FAILED: the table never reaches mode %d\n", m); return 1; }
    printf("FAST SCHEDULE OK: %ld launches (modes 0-4: %ld %ld %ld %ld %ld), %ld units, every (item, image) exactly once\n", launches, modes[0], modes[1], modes[2], modes[3], modes[4], units);
    return 0;
}
}  // namespace fastsched

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "fastplan")) return fastplan::run();
    if (argc > 1 && !strcmp(argv[1], "fastsched")) return fastsched::run();
    if (argc > 1 && !strcmp(argv[1], "refusals")) { const int rc = refusals::run(argc > 2 && !strcmp(argv[2], "list")); fflush(stdout); return rc; }      // (a failed run leaves its handle behind: its lines come before the leak report)
    if (argc > 3 && !strcmp(argv[1], "plan")) {                 // host_sanitize plan W H [nfeat scale levels [cell]]: the host-side plan of a geometry, or its refusal
        hs_orb_params p; hs_orb_default_params(&p);
        p.nfeatures = argc > 4 ? atoi(argv[4]) : 2000; if (argc > 5) p.scale_factor = (float)atof(argv[5]); if (argc > 6) p.nlevels = atoi(argv[6]);
        if (argc > 7) p.cell_px = atoi(argv[7]);
        hs_orb* ex = nullptr;
        CHECK(hs_orb_create(&p, 0, &ex) == HS_OK);
        const int rc = hs_orb_reserve(ex, atoi(argv[2]), atoi(argv[3]), 2);
        if (rc != HS_OK) { printf("refused: status %d: %s\n", rc, hs_orb_last_error(ex)); hs_orb_destroy(ex); return 0; }
        int32_t s[8]; hs_debug_plan_summary(ex, s);
        printf("pyramid launches: standard plan %d, small-batch plan %d (longest chain %d levels, %d B of LDS, %d workgroups per frame); FAST items per frame: %d wide, %d narrow; levels with quadtree keys: %d\n",
               s[0], s[1], s[5], s[6], s[7], s[2], s[3], s[4]);
        printf("plan digest: %016llx\n", (unsigned long long)hs_debug_plan_digest(ex));
        hs_orb_destroy(ex);
        return 0;
    }
    if (argc > 1 && !strcmp(argv[1], "threads")) {
        const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
        rng.seed(seed);
        CHECK(borrow_race() == 0);
        CHECK(frame_cache_section(seed) == 0);
        CHECK(threads_mode(seed) == 0);
        printf("HOST SANITIZE THREADS OK seed %llu; ", (unsigned long long)seed);
        print_counters("totals");
        return 0;
    }
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int n_geo = argc > 2 ? atoi(argv[2]) : 120, n_voc = argc > 3 ? atoi(argv[3]) : 400;
    rng.seed(seed);
    int ndev = 0;
    CHECK(hs_device_count(&ndev) == HS_OK && ndev == 1);

    // ---- geometry: the fixed shapes of the GPU suites, then the random sweep
    int accepted = 0, tried = 0;
    const int fixed[][7] = { {640, 480, 1000, 120, 8, 30, 2}, {1920, 1080, 2000, 120, 8, 30, 2}, {1920, 1080, 2000, 120, 8, 30, 32}, {4000, 3000, 3000, 140, 8, 30, 1},
                             {643, 481, 700, 120, 8, 30, 1}, {3840, 2160, 2000, 120, 8, 30, 1}, {2560, 40, 500, 120, 3, 30, 1}, {64, 64, 100, 120, 8, 30, 1}, {33, 33, 50, 200, 12, 12, 4},
                             {1200, 300, 1500, 120, 6, 30, 1}, {1900, 200, 1200, 120, 3, 30, 1}, {16384, 64, 100, 110, 2, 62, 1}, {1920, 1080, 9000, 120, 8, 30, 1}, {800, 600, 1500, 140, 8, 62, 2} };
    for (const auto& f : fixed) {
        const int r = geometry_case(f[0], f[1], f[2], f[3] / 100.f, f[4], f[5], f[6], (size_t)f[0] * f[1] * f[6] < 6000000);
        CHECK(r >= 0); accepted += r; tried++;
    }
    for (int i = 0; i < n_geo; i++) {
        // the tuning knobs that are PARSED (read once per handle): explicit pyramid plans incl. malformed ones, chain / deep-plan switches
        static const char* const plans[] = { "3,4", "2,5", "1,2,3,1", "7", "9,9", "1,1,1,1,1,1,1", "", "a,b", "2,,3", "0,0,0", "2,2,2,2,2,2,2,2,2,2", "-3,4" };
        if (i % 4 == 1) setenv("HS_PYRAMID_PLAN", plans[rnd(0, (int)(sizeof(plans) / sizeof(plans[0])) - 1)], 1); else unsetenv("HS_PYRAMID_PLAN");
        if (i % 7 == 2) setenv("HS_PYRAMID_CHAIN", rnd(0, 1) ? "2" : "0", 1); else unsetenv("HS_PYRAMID_CHAIN");
        if (i % 5 == 3) setenv("HS_PYRAMID_DEEP_MAX", rnd(0, 1) ? "0" : "100000", 1); else unsetenv("HS_PYRAMID_DEEP_MAX");
        const int w = rnd(1, 10) == 1 ? rnd(20, 120) : rnd(64, 2600), h = rnd(1, 10) == 1 ? rnd(20, 120) : rnd(64, 1600);
        const int r = geometry_case(w, h, rnd(20, 4000), 1.1f + 0.01f * (float)rnd(0, 90), rnd(1, 12), rnd(1, 8) == 1 ? rnd(8, 70) : 30, rnd(1, 5), (size_t)w * h < 1500000);
        CHECK(r >= 0); accepted += r; tried++;
    }
    unsetenv("HS_PYRAMID_PLAN"); unsetenv("HS_PYRAMID_CHAIN"); unsetenv("HS_PYRAMID_DEEP_MAX");
    CHECK(accepted > tried / 2);
    print_counters("HOST SANITIZE COUNTERS after the geometry sweep");       // (everything up to here is single-threaded: the same for every run of a commit)

    CHECK(borrow_race() == 0);
    CHECK(frame_cache_section(seed) == 0);

    print_counters("HOST SANITIZE COUNTERS after the threaded frame-cache section (varies from run to run)");
    CHECK(staged_sweep(12) == 0);

    // ---- vocabulary files: valid round trips, then truncations and random corruptions of both formats
    char dir[] = "/tmp/hs_host_sanitize_XXXXXX";
    CHECK(mkdtemp(dir) != nullptr);
    const std::string ptxt = std::string(dir) + "/v.txt", pbin = std::string(dir) + "/v.bin", pbad_t = std::string(dir) + "/bad.txt", pbad_b = std::string(dir) + "/bad.bin";
    std::vector<int32_t> cb, cc, word; std::vector<uint8_t> desc; std::vector<float> weight;
    hs_vocab* v = make_vocab(4, 3, cb, cc, desc, word, weight);
    CHECK(v != nullptr);
    CHECK(hs_vocab_save(v, ptxt.c_str()) == HS_OK && hs_vocab_save(v, pbin.c_str()) == HS_OK);
    hs_vocab_destroy(v);
    int loaded = 0, refused = 0;
    for (const std::string& p : { ptxt, pbin }) {
        hs_vocab* a = nullptr;
        CHECK(hs_vocab_load(p.c_str(), &a) == HS_OK && a && hs_vocab_last_error()[0] == 0);
        int32_t k, L, nn, nw, sc, wt;
        CHECK(hs_vocab_info(a, &k, &L, &nn, &nw, &sc, &wt) == HS_OK && k == 4 && L == 3 && nw == 64);
        hs_vocab_destroy(a);
    }
    CHECK(hs_vocab_load((std::string(dir) + "/missing.txt").c_str(), &v) != HS_OK && hs_vocab_last_error()[0] != 0);
    const std::vector<uint8_t> good_t = slurp(ptxt), good_b = slurp(pbin);
    CHECK(!good_t.empty() && !good_b.empty());
    for (int i = 0; i < n_voc; i++) {
        const bool text = i & 1;
        std::vector<uint8_t> b = text ? good_t : good_b;
        const int kind = rnd(0, 3);
        if (kind == 0) b.resize((size_t)rnd(0, (int)b.size()));                                                      // truncated
        else if (kind == 1) for (int j = 0, m = rnd(1, 8); j < m; j++) b[(size_t)rnd(0, (int)b.size() - 1)] = (uint8_t)rng();         // a few bytes
        else if (kind == 2) { const size_t at = (size_t)rnd(0, (int)b.size() - 1); for (size_t j = at; j < b.size() && j < at + 16; j++) b[j] = text ? (uint8_t)"9-.e 7"[rng() % 6] : (uint8_t)0xFF; }   // a run (huge numbers / counts)
        else { const size_t at = (size_t)rnd(0, (int)b.size()); b.insert(b.begin() + at, (size_t)rnd(1, 64), text ? (uint8_t)' ' : (uint8_t)rng()); }               // inserted bytes
        const std::string& p = text ? pbad_t : pbad_b;
        spit(p, b);
        hs_vocab* a = nullptr;
        const int st = hs_vocab_load(p.c_str(), &a);
        if (st == HS_OK) {                                                                                            // still well-formed: it must be usable
            CHECK(a != nullptr);
            hs_vocab_tree T; CHECK(hs_vocab_get_tree(a, &T) == HS_OK && T.n_nodes >= 2);
            hs_vocab_destroy(a); loaded++;
        } else { CHECK(a == nullptr && hs_vocab_last_error()[0] != 0); refused++; }
    }
    unlink(ptxt.c_str()); unlink(pbin.c_str()); unlink(pbad_t.c_str()); unlink(pbad_b.c_str()); rmdir(dir);
    printf("HOST SANITIZE OK seed %llu: %d of %d geometries configured, %ld kernel launches issued into the stub, %d corrupted vocabularies refused, %d still well-formed; ",
           (unsigned long long)seed, accepted, tried, hip_stub_launches(), refused, loaded);
    print_counters("totals");
    // (behind the line above, which earlier versions of this driver print too: what follows draws from the generator and issues launches)
    CHECK(map_sweep(12) == 0);
    CHECK(place_section() == 0);
    printf("HOST SANITIZE MAP OK seed %llu: key-frame graph, local map, pose optimiser, tracking / reference-key-frame / key-frame stages, place database; ", (unsigned long long)seed);
    print_counters("totals");
    return 0;
}
