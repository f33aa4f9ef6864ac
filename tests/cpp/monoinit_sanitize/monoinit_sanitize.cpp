// monoinit_sanitize.cpp — TEST: the host side of the monocular initialisation under AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_monoinit_abi.py), on the host-only objects of the library and hip_stub.cpp: hs_monoinit_check over one valid argument set and one
// knock-out at a time, "a refused call enqueues nothing" for both forms of hs_monoinit_estimate, and HsMonoWork carved over a block of exactly its
// stated size.
#include "hs_monoinit.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

extern "C" void hip_stub_counters(unsigned long long* out);
#define CHECK(c) do { if (!(c)) { printf("MONOINIT SANITIZE FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static hs_monoinit_params params(int its)
{
    hs_monoinit_params p{};
    p.fx = 500.f; p.fy = 500.f; p.cx = 320.f; p.cy = 240.f; p.sigma = 1.f; p.max_iterations = its; p.min_triangulated = 50; p.min_frac_triangulated = 0.9f;
    p.min_parallax_deg = 1.f; p.seed = 7;
    return p;
}
static bool same_counters(const unsigned long long* a, const unsigned long long* b) { return memcmp(a, b, 14 * sizeof(unsigned long long)) == 0; }

static int refusal_section()
{
    hs_orb_params op; hs_orb_default_params(&op);
    hs_orb* h = nullptr;
    CHECK(hs_orb_create(&op, 0, &h) == HS_OK);
    const int Q = 3, cap = 2;
    std::vector<hs_monoinit_params> par = { params(12), params(200), params(3) };
    std::vector<int64_t> off1 = { 0, 40, 49, 120 }, off2 = { 0, 50, 50, 130 };
    std::vector<hs_keypoint> k1(120), k2(130);
    for (size_t i = 0; i < k1.size(); i++) { k1[i] = hs_keypoint{}; k1[i].x = (float)(i * 5 % 640); k1[i].y = (float)(i * 7 % 480); }
    for (size_t i = 0; i < k2.size(); i++) { k2[i] = hs_keypoint{}; k2[i].x = (float)(i * 11 % 640); k2[i].y = (float)(i * 3 % 480); }
    std::vector<int32_t> m(120);
    for (size_t i = 0; i < m.size(); i++) m[i] = i % 3 == 0 ? -1 : (int32_t)(i % 50);
    std::vector<uint32_t> draws((size_t)Q * cap * HS_MONOINIT_DRAW_STRIDE, 0u);
    std::vector<hs_monoinit_result> res(Q);
    std::vector<uint8_t> ih(120), jf(120), tri(120);
    std::vector<float> p3d(360);
    CHECK(hs_monoinit_check(Q, par.data(), off1.data(), k1.data(), off2.data(), k2.data(), m.data(), draws.data(), cap, res.data(), ih.data(), jf.data(), p3d.data(),
                            tri.data(), 0, nullptr) == nullptr);
    CHECK(hs_monoinit_estimate(h, Q, par.data(), off1.data(), k1.data(), off2.data(), k2.data(), m.data(), draws.data(), cap, res.data(), ih.data(), jf.data(), p3d.data(),
                               tri.data()) == HS_OK);
    CHECK(hs_monoinit_call_bound(Q, par.data()) == 200 && hs_monoinit_work_bytes(Q, 120, 200) == HsMonoWork::bytes(Q, 120, 200));
    void *d_k1, *d_k2, *d_m, *d_draws, *d_res, *d_ih, *d_if, *d_p3d, *d_tri, *d_work;
    CHECK(hs_device_alloc(h, k1.size() * sizeof(hs_keypoint), &d_k1) == HS_OK && hs_device_alloc(h, k2.size() * sizeof(hs_keypoint), &d_k2) == HS_OK &&
          hs_device_alloc(h, 480, &d_m) == HS_OK && hs_device_alloc(h, draws.size() * 4, &d_draws) == HS_OK && hs_device_alloc(h, Q * sizeof(hs_monoinit_result), &d_res) == HS_OK &&
          hs_device_alloc(h, 120, &d_ih) == HS_OK && hs_device_alloc(h, 120, &d_if) == HS_OK && hs_device_alloc(h, 1440, &d_p3d) == HS_OK &&
          hs_device_alloc(h, 120, &d_tri) == HS_OK && hs_device_alloc(h, hs_monoinit_work_bytes(Q, 120, 200), &d_work) == HS_OK);
    CHECK(hs_monoinit_estimate_device(h, Q, par.data(), off1.data(), (hs_keypoint*)d_k1, off2.data(), (hs_keypoint*)d_k2, (int32_t*)d_m, (uint32_t*)d_draws, cap,
                                      (hs_monoinit_result*)d_res, (uint8_t*)d_ih, (uint8_t*)d_if, (float*)d_p3d, (uint8_t*)d_tri, d_work, nullptr) == HS_OK);
    // knock-outs: one argument at a time; across a refused call the stub counts no launch, copy, memset or allocation
    std::vector<int64_t> dec = { 0, 40, 39, 120 }, neg = { -1, 40, 49, 120 }, big = { 0, 40, 49, 49 + (int64_t)2147483648LL };
    const float nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<std::vector<hs_monoinit_params>> bad_par;
    for (int k = 0; k < 9; k++) {
        std::vector<hs_monoinit_params> b = par;
        switch (k) {
        case 0: b[1].max_iterations = 0; break;   case 1: b[2].max_iterations = HS_MONOINIT_MAX_ITERATIONS + 1; break;   case 2: b[0].sigma = 0.f; break;
        case 3: b[0].sigma = nan; break;          case 4: b[1].fx = -1.f; break;                                         case 5: b[2].min_parallax_deg = 0.f; break;
        case 6: b[2].min_parallax_deg = 180.f; break; case 7: b[0].min_frac_triangulated = nan; break;                    case 8: b[1].min_triangulated = -1; break;
        }
        bad_par.push_back(b);
    }
    int refused = 0;
    for (int form = 0; form < 2; form++)
        for (int k = 0; k < 28; k++) {
            int q = Q, c = cap;
            const hs_monoinit_params* pp = par.data(); const int64_t *po1 = off1.data(), *po2 = off2.data();
            const hs_keypoint *pk1 = form ? (hs_keypoint*)d_k1 : k1.data(), *pk2 = form ? (hs_keypoint*)d_k2 : k2.data();
            const int32_t* pm = form ? (int32_t*)d_m : m.data(); const uint32_t* pd = form ? (uint32_t*)d_draws : draws.data();
            hs_monoinit_result* pr = form ? (hs_monoinit_result*)d_res : res.data();
            uint8_t *pih = form ? (uint8_t*)d_ih : ih.data(), *pif = form ? (uint8_t*)d_if : jf.data(), *pt = form ? (uint8_t*)d_tri : tri.data();
            float* p3 = form ? (float*)d_p3d : p3d.data();
            void* pw = d_work; hs_orb* hh = h;
            bool device_only = false;
            switch (k) {
            case 0: hh = nullptr; break;   case 1: q = 0; break;           case 2: pp = nullptr; break;    case 3: po1 = nullptr; break;   case 4: po2 = nullptr; break;
            case 5: pk1 = nullptr; break;  case 6: pk2 = nullptr; break;   case 7: pm = nullptr; break;    case 8: pd = nullptr; break;    case 9: c = -1; break;
            case 10: pr = nullptr; break;  case 11: pih = nullptr; break;  case 12: pif = nullptr; break;  case 13: p3 = nullptr; break;   case 14: pt = nullptr; break;
            case 15: po1 = dec.data(); break; case 16: po2 = neg.data(); break; case 17: po1 = big.data(); break;
            case 18: case 19: case 20: case 21: case 22: case 23: case 24: case 25: case 26: pp = bad_par[k - 18].data(); break;
            case 27: device_only = true; pw = (char*)d_work + 8; break;
            }
            if (device_only && !form) continue;
            unsigned long long a[16], b[16];
            hip_stub_counters(a);
            const int rc = form ? hs_monoinit_estimate_device(hh, q, pp, po1, pk1, po2, pk2, pm, pd, c, pr, pih, pif, p3, pt, pw, nullptr)
                                : hs_monoinit_estimate(hh, q, pp, po1, pk1, po2, pk2, pm, pd, c, pr, pih, pif, p3, pt);
            hip_stub_counters(b);
            CHECK(rc == HS_ERR_INVALID && same_counters(a, b));
            if (k > 0) CHECK(hs_monoinit_check(q, pp, po1, pk1, po2, pk2, pm, pd, c, pr, pih, pif, p3, pt, form, pw) != nullptr);
            refused++;
        }
    {   // the device form alone: no work area, misaligned key points
        unsigned long long a[16], b[16];
        hip_stub_counters(a);
        CHECK(hs_monoinit_estimate_device(h, Q, par.data(), off1.data(), (hs_keypoint*)d_k1, off2.data(), (hs_keypoint*)d_k2, (int32_t*)d_m, nullptr, 0, (hs_monoinit_result*)d_res,
                                          (uint8_t*)d_ih, (uint8_t*)d_if, (float*)d_p3d, (uint8_t*)d_tri, nullptr, nullptr) == HS_ERR_INVALID);
        CHECK(hs_monoinit_estimate_device(h, Q, par.data(), off1.data(), (hs_keypoint*)((char*)d_k1 + 8), off2.data(), (hs_keypoint*)d_k2, (int32_t*)d_m, nullptr, 0,
                                          (hs_monoinit_result*)d_res, (uint8_t*)d_ih, (uint8_t*)d_if, (float*)d_p3d, (uint8_t*)d_tri, d_work, nullptr) == HS_ERR_INVALID);
        CHECK(hs_monoinit_estimate_device(h, Q, par.data(), off1.data(), (hs_keypoint*)d_k1, off2.data(), (hs_keypoint*)((char*)d_k2 + 8), (int32_t*)d_m, nullptr, 0,
                                          (hs_monoinit_result*)d_res, (uint8_t*)d_ih, (uint8_t*)d_if, (float*)d_p3d, (uint8_t*)d_tri, d_work, nullptr) == HS_ERR_INVALID);
        hip_stub_counters(b);
        CHECK(same_counters(a, b));
        refused += 3;
    }
    for (void* p : { d_k1, d_k2, d_m, d_draws, d_res, d_ih, d_if, d_p3d, d_tri, d_work }) CHECK(hs_device_free(h, p) == HS_OK);
    hs_orb_destroy(h);
    printf("refusals: %d refused calls enqueued nothing\n", refused);
    return 0;
}

static int layout_section()
{
    long n = 0;
    for (int Q : { 0, 1, 3, 17 }) for (long long nt : { 0LL, 1LL, 9LL, 65LL, 1000LL }) for (int H : { 0, 1, 12, 200 }) {
        const size_t bytes = HsMonoWork::bytes(Q, nt, H);
        CHECK(bytes == hs_monoinit_work_bytes(Q, nt, H) && bytes >= 256);
        char* block = (char*)malloc(bytes);                        // exactly the stated size: AddressSanitizer sees a store past it
        HsWorkCursor cur(block);
        HsMonoWork w(cur, Q, nt, H);
        const size_t nh = (size_t)Q * 2 * H;
        for (int q = 0; q < Q; q++) w.n[q] = 7;
        for (size_t i = 0; i < (size_t)Q * HS_MONO_PREP_WORDS; i++) w.prep[i] = 1.f;
        for (long long i = 0; i < nt; i++) { w.m1[i] = 1; w.m2[i] = 2; w.cosv[i] = 3.f; }
        for (size_t i = 0; i < nh; i++) w.score[i] = 4.f;
        for (size_t i = 0; i < nh * HS_MONO_MODEL_WORDS; i++) w.model[i] = 5.f;
        for (int q = 0; q < Q; q++) CHECK(w.n[q] == 7);
        for (long long i = 0; i < nt; i++) CHECK(w.m1[i] == 1 && w.m2[i] == 2 && w.cosv[i] == 3.f);
        for (size_t i = 0; i < nh; i++) CHECK(w.score[i] == 4.f);
        for (size_t i = 0; i < nh * HS_MONO_MODEL_WORDS; i++) CHECK(w.model[i] == 5.f);
        CHECK(((uintptr_t)w.model - (uintptr_t)block) % 256 == 0 && ((uintptr_t)w.cosv - (uintptr_t)block) % 256 == 0 && cur.offset() == bytes);
        free(block);
        n++;
    }
    CHECK(HsMonoWork::bytes(-1, -5, -2) == HsMonoWork::bytes(0, 0, 0));
    printf("layout: %ld carves\n", n);
    return 0;
}

int main()
{
    if (refusal_section() || layout_section()) return 1;
    printf("MONOINIT SANITIZE OK\n");
    return 0;
}
