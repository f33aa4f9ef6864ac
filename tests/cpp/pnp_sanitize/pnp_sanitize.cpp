// pnp_sanitize.cpp — TEST: the host side of the batched EPnP RANSAC under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_pnp_abi.py), on
// the host-only objects of the library and hip_stub.cpp: hs_pnp_plan over ordinary and degenerate parameters, "a refused call enqueues nothing" for
// both forms of hs_pnp_iterate (one valid argument set, one knock-out at a time), and HsPnpWork carved over a block of exactly its stated size.
#include "hs_pnp.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

extern "C" void hip_stub_counters(unsigned long long* out);
#define CHECK(c) do { if (!(c)) { printf("PNP SANITIZE FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static hs_pnp_params params(double p, int mi, int mx, int ms, float eps)
{
    hs_pnp_params q{};
    q.probability = p; q.min_inliers = mi; q.max_iterations = mx; q.min_set = ms; q.epsilon = eps; q.th2 = 5.991f;
    q.fx = 520.f; q.fy = 515.f; q.cx = 320.5f; q.cy = 240.25f; q.seed = 7;
    return q;
}

static int plan_section()
{
    struct { int N, mx, min_inliers; float eps; int its; } known[] = { { 100, 300, 50, 0.5f, 35 }, { 16, 300, 10, 0.625f, 17 }, { 10, 300, 10, 1.0f, 1 }, { 100, 20, 50, 0.5f, 20 } };
    for (auto& k : known) {
        hs_pnp_params p = params(0.99, 10, k.mx, 4, 0.5f);
        hs_pnp_plan_t plan;
        CHECK(hs_pnp_plan(k.N, &p, &plan) == HS_OK && plan.min_inliers == k.min_inliers && plan.epsilon == k.eps && plan.max_iterations == k.its);
    }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float epss[] = { 0.f, 1e-30f, 0.5f, 1.f, 2.f, 1e30f, inf, -inf, nan, -0.5f };
    const double probs[] = { 0.0, 0.5, 0.99, 1.0, 2.0, -1.0, (double)nan, (double)inf };
    const int Ns[] = { 0, 1, 3, 4, 10, 100, 2147483647 };
    const int mxs[] = { -5, 0, 1, 300, 2147483647 };
    long n = 0;
    for (float e : epss) for (double pr : probs) for (int N : Ns) for (int mx : mxs) for (int mi : { -3, 0, 10, 2147483647 }) {
        hs_pnp_params p = params(pr, mi, mx, 4, e);
        hs_pnp_plan_t plan;
        CHECK(hs_pnp_plan(N, &p, &plan) == HS_OK);
        CHECK(plan.max_iterations >= 1 && plan.min_inliers >= 4 && (mx < 1 || plan.max_iterations <= mx));
        n++;
    }
    hs_pnp_params p = params(0.99, 10, 300, 3, 0.5f);
    hs_pnp_plan_t plan;
    CHECK(hs_pnp_plan(100, &p, &plan) == HS_ERR_INVALID && hs_pnp_plan(-1, &p, &plan) == HS_ERR_INVALID);
    p.min_set = 4;
    CHECK(hs_pnp_plan(100, nullptr, &plan) == HS_ERR_INVALID && hs_pnp_plan(100, &p, nullptr) == HS_ERR_INVALID);
    hs_pnp_state st; memset(&st, 0x55, sizeof st);
    hs_pnp_state_init(&st); hs_pnp_state_init(nullptr);
    CHECK(st.iterations == 0 && st.best_inliers == 0 && st.best_Tcw[15] == 0.f);
    printf("plan: %ld parameter sets\n", n);
    return 0;
}

static bool same_counters(const unsigned long long* a, const unsigned long long* b) { return memcmp(a, b, 14 * sizeof(unsigned long long)) == 0; }

static int refusal_section()
{
    hs_orb_params op; hs_orb_default_params(&op);
    hs_orb* h = nullptr;
    CHECK(hs_orb_create(&op, 0, &h) == HS_OK);
    const int Q = 3, n_it = 5, cap = 2;
    std::vector<hs_pnp_params> par = { params(0.99, 10, 12, 4, 0.5f), params(0.99, 10, 12, 6, 0.5f), params(0.99, 10, 3, 4, 0.5f) };
    std::vector<int64_t> off = { 0, 40, 49, 120 };
    std::vector<hs_pnp_corr> corrs(120);
    for (size_t i = 0; i < corrs.size(); i++) corrs[i] = hs_pnp_corr{ { (float)i, 1.f, 5.f }, 10.f, 20.f, 1.f, (int32_t)i, 0 };
    std::vector<uint32_t> draws((size_t)Q * cap * HS_PNP_MAX_SET, 0u);
    std::vector<hs_pnp_state> states(Q); for (auto& s : states) hs_pnp_state_init(&s);
    std::vector<uint8_t> best(120), inl(120);
    std::vector<hs_pnp_result> res(Q);
    CHECK(hs_pnp_iterate(h, Q, par.data(), off.data(), corrs.data(), n_it, draws.data(), cap, states.data(), best.data(), res.data(), inl.data()) == HS_OK);
    CHECK(hs_pnp_iterate(h, Q, par.data(), off.data(), corrs.data(), n_it, nullptr, 0, states.data(), best.data(), res.data(), inl.data()) == HS_OK);
    const int H = hs_pnp_call_bound(Q, par.data(), off.data(), n_it);
    CHECK(H == 12 && hs_pnp_work_bytes(Q, 120, H) == HsPnpWork::bytes(Q, 120, H));
    void *d_corrs, *d_draws, *d_states, *d_best, *d_inl, *d_res, *d_work;
    CHECK(hs_device_alloc(h, corrs.size() * 32, &d_corrs) == HS_OK && hs_device_alloc(h, draws.size() * 4, &d_draws) == HS_OK && hs_device_alloc(h, Q * sizeof(hs_pnp_state), &d_states) == HS_OK &&
          hs_device_alloc(h, 120, &d_best) == HS_OK && hs_device_alloc(h, 120, &d_inl) == HS_OK && hs_device_alloc(h, Q * sizeof(hs_pnp_result), &d_res) == HS_OK &&
          hs_device_alloc(h, hs_pnp_work_bytes(Q, 120, H), &d_work) == HS_OK);
    CHECK(hs_pnp_iterate_device(h, Q, par.data(), off.data(), (hs_pnp_corr*)d_corrs, n_it, (uint32_t*)d_draws, cap, (hs_pnp_state*)d_states, (uint8_t*)d_best,
                                (hs_pnp_result*)d_res, (uint8_t*)d_inl, d_work, nullptr) == HS_OK);
    // knock-outs: one argument at a time; across a refused call the stub counts no launch, copy, memset or allocation
    std::vector<int64_t> dec = { 0, 40, 39, 120 }, neg = { -1, 40, 49, 120 };
    std::vector<hs_pnp_params> small_set = par, big_set = par;
    small_set[1].min_set = 3; big_set[2].min_set = HS_PNP_MAX_SET + 1;
    int refused = 0;
    for (int form = 0; form < 2; form++)
        for (int k = 0; k < 16; k++) {
            int q = Q, n = n_it, c = cap;
            const hs_pnp_params* pp = par.data(); const int64_t* po = off.data();
            const hs_pnp_corr* pc = form ? (hs_pnp_corr*)d_corrs : corrs.data(); const uint32_t* pd = form ? (uint32_t*)d_draws : draws.data();
            hs_pnp_state* ps = form ? (hs_pnp_state*)d_states : states.data(); uint8_t* pb = form ? (uint8_t*)d_best : best.data();
            hs_pnp_result* pr = form ? (hs_pnp_result*)d_res : res.data(); uint8_t* pi = form ? (uint8_t*)d_inl : inl.data();
            void* pw = d_work; hs_orb* hh = h;
            switch (k) {
            case 0: hh = nullptr; break;  case 1: q = 0; break;         case 2: pp = nullptr; break;     case 3: po = nullptr; break;
            case 4: pc = nullptr; break;  case 5: n = 0; break;         case 6: pd = nullptr; break;     case 7: c = -1; break;
            case 8: ps = nullptr; break;  case 9: pb = nullptr; break;  case 10: pr = nullptr; break;    case 11: pi = nullptr; break;
            case 12: po = dec.data(); break; case 13: po = neg.data(); break; case 14: pp = small_set.data(); break; case 15: pp = big_set.data(); break;
            }
            unsigned long long a[16], b[16];
            hip_stub_counters(a);
            const int rc = form ? hs_pnp_iterate_device(hh, q, pp, po, pc, n, pd, c, ps, pb, pr, pi, pw, nullptr) : hs_pnp_iterate(hh, q, pp, po, pc, n, pd, c, ps, pb, pr, pi);
            hip_stub_counters(b);
            CHECK(rc == HS_ERR_INVALID && same_counters(a, b));
            refused++;
        }
    {   // the device form alone: no work area, a misaligned one, misaligned correspondences
        unsigned long long a[16], b[16];
        hip_stub_counters(a);
        CHECK(hs_pnp_iterate_device(h, Q, par.data(), off.data(), (hs_pnp_corr*)d_corrs, n_it, nullptr, 0, (hs_pnp_state*)d_states, (uint8_t*)d_best, (hs_pnp_result*)d_res,
                                    (uint8_t*)d_inl, nullptr, nullptr) == HS_ERR_INVALID);
        CHECK(hs_pnp_iterate_device(h, Q, par.data(), off.data(), (hs_pnp_corr*)d_corrs, n_it, nullptr, 0, (hs_pnp_state*)d_states, (uint8_t*)d_best, (hs_pnp_result*)d_res,
                                    (uint8_t*)d_inl, (char*)d_work + 8, nullptr) == HS_ERR_INVALID);
        CHECK(hs_pnp_iterate_device(h, Q, par.data(), off.data(), (hs_pnp_corr*)((char*)d_corrs + 8), n_it, nullptr, 0, (hs_pnp_state*)d_states, (uint8_t*)d_best,
                                    (hs_pnp_result*)d_res, (uint8_t*)d_inl, d_work, nullptr) == HS_ERR_INVALID);
        hip_stub_counters(b);
        CHECK(same_counters(a, b));
        refused += 3;
    }
    for (void* p : { d_corrs, d_draws, d_states, d_best, d_inl, d_res, d_work }) CHECK(hs_device_free(h, p) == HS_OK);
    hs_orb_destroy(h);
    printf("refusals: %d refused calls enqueued nothing\n", refused);
    return 0;
}

static int layout_section()
{
    long n = 0;
    size_t last = 0;
    for (int Q : { 0, 1, 3, 17 }) for (long long nt : { 0LL, 1LL, 9LL, 65LL, 1000LL }) for (int H : { 0, 1, 12, 300 }) {
        const size_t bytes = HsPnpWork::bytes(Q, nt, H);
        CHECK(bytes == hs_pnp_work_bytes(Q, nt, H) && bytes >= 256);
        char* block = (char*)malloc(bytes);                        // exactly the stated size: AddressSanitizer sees a store past it
        HsWorkCursor cur(block);
        HsPnpWork w(cur, Q, nt, H);
        const size_t nh = (size_t)Q * H;
        for (size_t i = 0; i < nh * 12; i++) w.hyp_pose[i] = 1.0;
        for (size_t i = 0; i < (size_t)nt * 5; i++) w.pts[i] = 2.0;
        for (size_t i = 0; i < nh; i++) w.hyp_count[i] = 3;
        for (size_t i = 0; i < (size_t)nt; i++) w.tmp_mask[i] = 4;
        for (size_t i = 0; i < nh * 12; i++) CHECK(w.hyp_pose[i] == 1.0);
        for (size_t i = 0; i < (size_t)nt * 5; i++) CHECK(w.pts[i] == 2.0);
        for (size_t i = 0; i < nh; i++) CHECK(w.hyp_count[i] == 3);
        CHECK(((uintptr_t)w.hyp_pose - (uintptr_t)block) % 256 == 0 && ((uintptr_t)w.pts - (uintptr_t)block) % 256 == 0 && cur.offset() == bytes);
        free(block);
        n++; last = bytes;
    }
    CHECK(HsPnpWork::bytes(-1, -5, -2) == HsPnpWork::bytes(0, 0, 0) && last > 0);
    printf("layout: %ld carves\n", n);
    return 0;
}

int main()
{
    if (plan_section() || refusal_section() || layout_section()) return 1;
    printf("PNP SANITIZE OK\n");
    return 0;
}
