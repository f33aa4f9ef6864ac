// sim3_sanitize.cpp — TEST: the host side of the batched Horn Sim3 RANSAC under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_sim3_abi.py),
// on the host-only objects of the library and hip_stub.cpp: hs_sim3_plan over ordinary and degenerate parameters, "a refused call enqueues nothing"
// for both forms of hs_sim3_iterate (one valid argument set, one knock-out at a time), and HsSim3Work carved over a block of exactly its stated size.
#include "hs_sim3.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

extern "C" void hip_stub_counters(unsigned long long* out);
#define CHECK(c) do { if (!(c)) { printf("SIM3 SANITIZE FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static hs_sim3_params params(double p, int mi, int mx)
{
    hs_sim3_params q{};
    q.probability = p; q.min_inliers = mi; q.max_iterations = mx; q.fix_scale = 0;
    q.fx1 = 520.f; q.fy1 = 515.f; q.cx1 = 320.5f; q.cy1 = 240.25f; q.fx2 = 458.f; q.fy2 = 457.5f; q.cx2 = 367.25f; q.cy2 = 248.5f; q.seed = 7;
    return q;
}

static int plan_section()
{
    struct { int N, mi, mx, its; float eps; } known[] = { { 100, 20, 300, 300, 0.2f }, { 100, 20, 1000000, 574, 0.2f }, { 20, 20, 300, 1, 1.0f }, { 40, 20, 300, 35, 0.5f },
                                                          { 100, 0, 300, 1, 0.0f }, { 100, 20, 0, 1, 0.2f } };
    for (auto& k : known) {
        hs_sim3_params p = params(0.99, k.mi, k.mx);
        hs_sim3_plan_t plan;
        CHECK(hs_sim3_plan(k.N, &p, &plan) == HS_OK && plan.max_iterations == k.its && plan.epsilon == k.eps);
    }
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double probs[] = { 0.0, 0.5, 0.99, 1.0, 2.0, -1.0, nan, inf };
    const int Ns[] = { 0, 1, 2, 3, 10, 100, 2147483647 };
    const int mxs[] = { -5, 0, 1, 300, 2147483647 };
    long n = 0;
    for (double pr : probs) for (int N : Ns) for (int mx : mxs) for (int mi : { -3, 0, 1, 3, 10, 100, 2147483647 }) {
        hs_sim3_params p = params(pr, mi, mx);
        hs_sim3_plan_t plan;
        CHECK(hs_sim3_plan(N, &p, &plan) == HS_OK);
        CHECK(plan.max_iterations >= 1 && (mx < 1 || plan.max_iterations <= mx));
        n++;
    }
    hs_sim3_params p = params(0.99, 20, 300);
    hs_sim3_plan_t plan;
    CHECK(hs_sim3_plan(-1, &p, &plan) == HS_ERR_INVALID && hs_sim3_plan(100, nullptr, &plan) == HS_ERR_INVALID && hs_sim3_plan(100, &p, nullptr) == HS_ERR_INVALID);
    hs_sim3_state st; memset(&st, 0x55, sizeof st);
    hs_sim3_state_init(&st); hs_sim3_state_init(nullptr);
    CHECK(st.iterations == 0 && st.best_inliers == 0 && st.T12[15] == 0.f && st.s == 0.f);
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
    std::vector<hs_sim3_params> par = { params(0.99, 10, 12), params(0.99, 3, 300), params(0.99, 60, 3) };
    std::vector<int64_t> off = { 0, 40, 49, 120 };
    std::vector<hs_sim3_corr> corrs(120);
    for (size_t i = 0; i < corrs.size(); i++) {
        hs_sim3_corr c{};
        c.X1c[0] = (float)i; c.X1c[1] = 1.f; c.X1c[2] = 5.f; c.X2c[0] = 1.f; c.X2c[1] = (float)i; c.X2c[2] = 4.f; c.sigma2_1 = 1.f; c.sigma2_2 = 1.44f; c.idx1 = (int32_t)i;
        corrs[i] = c;
    }
    std::vector<uint32_t> draws((size_t)Q * cap * HS_SIM3_DRAW_STRIDE, 0u);
    std::vector<hs_sim3_state> states(Q); for (auto& s : states) hs_sim3_state_init(&s);
    std::vector<uint8_t> best(120), inl(120);
    std::vector<hs_sim3_result> res(Q);
    CHECK(hs_sim3_iterate(h, Q, par.data(), off.data(), corrs.data(), n_it, draws.data(), cap, states.data(), best.data(), res.data(), inl.data()) == HS_OK);
    CHECK(hs_sim3_iterate(h, Q, par.data(), off.data(), corrs.data(), n_it, nullptr, 0, states.data(), best.data(), res.data(), inl.data()) == HS_OK);
    const int H = hs_sim3_call_bound(Q, par.data(), off.data(), n_it);
    CHECK(H == 5 && hs_sim3_call_bound(Q, par.data(), off.data(), 1) == 1 && hs_sim3_work_bytes(Q, 120, H) == HsSim3Work::bytes(Q, 120, H));
    void *d_corrs, *d_draws, *d_states, *d_best, *d_inl, *d_res, *d_work;
    CHECK(hs_device_alloc(h, corrs.size() * sizeof(hs_sim3_corr), &d_corrs) == HS_OK && hs_device_alloc(h, draws.size() * 4, &d_draws) == HS_OK &&
          hs_device_alloc(h, Q * sizeof(hs_sim3_state), &d_states) == HS_OK && hs_device_alloc(h, 120, &d_best) == HS_OK && hs_device_alloc(h, 120, &d_inl) == HS_OK &&
          hs_device_alloc(h, Q * sizeof(hs_sim3_result), &d_res) == HS_OK && hs_device_alloc(h, hs_sim3_work_bytes(Q, 120, H), &d_work) == HS_OK);
    CHECK(hs_sim3_iterate_device(h, Q, par.data(), off.data(), (hs_sim3_corr*)d_corrs, n_it, (uint32_t*)d_draws, cap, (hs_sim3_state*)d_states, (uint8_t*)d_best,
                                 (hs_sim3_result*)d_res, (uint8_t*)d_inl, d_work, nullptr) == HS_OK);
    // knock-outs: one argument at a time; across a refused call the stub counts no launch, copy, memset or allocation
    std::vector<int64_t> dec = { 0, 40, 39, 120 }, neg = { -1, 40, 49, 120 }, big = { 0, 40, 49, 49 + (int64_t)2147483648LL };
    std::vector<hs_sim3_params> neg_min = par;
    neg_min[1].min_inliers = -1;
    int refused = 0;
    for (int form = 0; form < 2; form++)
        for (int k = 0; k < 16; k++) {
            int q = Q, n = n_it, c = cap;
            const hs_sim3_params* pp = par.data(); const int64_t* po = off.data();
            const hs_sim3_corr* pc = form ? (hs_sim3_corr*)d_corrs : corrs.data(); const uint32_t* pd = form ? (uint32_t*)d_draws : draws.data();
            hs_sim3_state* ps = form ? (hs_sim3_state*)d_states : states.data(); uint8_t* pb = form ? (uint8_t*)d_best : best.data();
            hs_sim3_result* pr = form ? (hs_sim3_result*)d_res : res.data(); uint8_t* pi = form ? (uint8_t*)d_inl : inl.data();
            void* pw = d_work; hs_orb* hh = h;
            switch (k) {
            case 0: hh = nullptr; break;  case 1: q = 0; break;         case 2: pp = nullptr; break;     case 3: po = nullptr; break;
            case 4: pc = nullptr; break;  case 5: n = 0; break;         case 6: pd = nullptr; break;     case 7: c = -1; break;
            case 8: ps = nullptr; break;  case 9: pb = nullptr; break;  case 10: pr = nullptr; break;    case 11: pi = nullptr; break;
            case 12: po = dec.data(); break; case 13: po = neg.data(); break; case 14: pp = neg_min.data(); break; case 15: po = big.data(); break;
            }
            unsigned long long a[16], b[16];
            hip_stub_counters(a);
            const int rc = form ? hs_sim3_iterate_device(hh, q, pp, po, pc, n, pd, c, ps, pb, pr, pi, pw, nullptr) : hs_sim3_iterate(hh, q, pp, po, pc, n, pd, c, ps, pb, pr, pi);
            hip_stub_counters(b);
            CHECK(rc == HS_ERR_INVALID && same_counters(a, b));
            refused++;
        }
    {   // the host form alone: a state with a negative count
        std::vector<hs_sim3_state> bad = states;
        bad[2].best_inliers = -1;
        unsigned long long a[16], b[16];
        hip_stub_counters(a);
        CHECK(hs_sim3_iterate(h, Q, par.data(), off.data(), corrs.data(), n_it, nullptr, 0, bad.data(), best.data(), res.data(), inl.data()) == HS_ERR_INVALID);
        bad = states; bad[0].iterations = -7;
        CHECK(hs_sim3_iterate(h, Q, par.data(), off.data(), corrs.data(), n_it, nullptr, 0, bad.data(), best.data(), res.data(), inl.data()) == HS_ERR_INVALID);
        hip_stub_counters(b);
        CHECK(same_counters(a, b));
        refused += 2;
    }
    {   // the device form alone: no work area, a misaligned one, misaligned correspondences
        unsigned long long a[16], b[16];
        hip_stub_counters(a);
        CHECK(hs_sim3_iterate_device(h, Q, par.data(), off.data(), (hs_sim3_corr*)d_corrs, n_it, nullptr, 0, (hs_sim3_state*)d_states, (uint8_t*)d_best, (hs_sim3_result*)d_res,
                                     (uint8_t*)d_inl, nullptr, nullptr) == HS_ERR_INVALID);
        CHECK(hs_sim3_iterate_device(h, Q, par.data(), off.data(), (hs_sim3_corr*)d_corrs, n_it, nullptr, 0, (hs_sim3_state*)d_states, (uint8_t*)d_best, (hs_sim3_result*)d_res,
                                     (uint8_t*)d_inl, (char*)d_work + 8, nullptr) == HS_ERR_INVALID);
        CHECK(hs_sim3_iterate_device(h, Q, par.data(), off.data(), (hs_sim3_corr*)((char*)d_corrs + 8), n_it, nullptr, 0, (hs_sim3_state*)d_states, (uint8_t*)d_best,
                                     (hs_sim3_result*)d_res, (uint8_t*)d_inl, d_work, nullptr) == HS_ERR_INVALID);
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
        const size_t bytes = HsSim3Work::bytes(Q, nt, H);
        CHECK(bytes == hs_sim3_work_bytes(Q, nt, H) && bytes >= 256);
        char* block = (char*)malloc(bytes);                        // exactly the stated size: AddressSanitizer sees a store past it
        HsWorkCursor cur(block);
        HsSim3Work w(cur, Q, nt, H);
        const size_t nh = (size_t)Q * H;
        for (size_t i = 0; i < nh * HS_SIM3_POSE_WORDS; i++) w.hyp_pose[i] = 1.f;
        for (size_t i = 0; i < nh; i++) w.hyp_count[i] = 3;
        for (size_t i = 0; i < nh * HS_SIM3_POSE_WORDS; i++) CHECK(w.hyp_pose[i] == 1.f);
        for (size_t i = 0; i < nh; i++) CHECK(w.hyp_count[i] == 3);
        CHECK(((uintptr_t)w.hyp_pose - (uintptr_t)block) % 256 == 0 && ((uintptr_t)w.hyp_count - (uintptr_t)block) % 256 == 0 && cur.offset() == bytes);
        free(block);
        n++; last = bytes;
    }
    CHECK(HsSim3Work::bytes(-1, -5, -2) == HsSim3Work::bytes(0, 0, 0) && last > 0);
    printf("layout: %ld carves\n", n);
    return 0;
}

int main()
{
    if (plan_section() || refusal_section() || layout_section()) return 1;
    printf("SIM3 SANITIZE OK\n");
    return 0;
}
