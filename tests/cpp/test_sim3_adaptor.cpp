// HipSim3Solver (hyslam_amd/host/HipSim3Solver.h) on the cv_compat.h stand-ins against the C ABI: the same candidates through the adaptor (KeyFrame,
// FeatureViews, Camera, MapPoint objects; matches with null entries, null own points, bad landmarks and landmarks a key frame does not see) and
// through hs_sim3_iterate on hand-gathered arrays must give identical bytes — pose, flag of every match, nInliers, bNoMore, the estimates — alone,
// all in one static call, and on a second call (the state persists).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "../../hyslam_amd/host/HipSim3Solver.h"

using namespace HYSLAM;

static uint32_t rng_state;
static float rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (float)((rng_state >> 8) & 0xFFFF) / 65536.0f; }

struct World {
    std::vector<std::unique_ptr<MapPoint>> lms;
    std::unique_ptr<KeyFrame> kf1, kf2;
    std::vector<MapPoint*> matched12;
    std::vector<int> expect_idx1;                                  // the i1 the constructor must keep, in order
};

static cv::Mat pose(float angle, float tx, float ty, float tz)
{
    cv::Mat T(4, 4, CV_32F);
    const float c = std::cos(angle), s = std::sin(angle);
    const float v[16] = { c, 0, s, tx, 0, 1, 0, ty, -s, 0, c, tz, 0, 0, 0, 1 };
    for (int i = 0; i < 16; i++) T.at<float>(i / 4, i % 4) = v[i];
    return T;
}

// n matches; key frame 1 sees world A, key frame 2 world B = a similarity of A (scale `scale`), a share of the matches wrong
static void build(World& W, int n, float outlier_share, float scale, uint32_t seed)
{
    rng_state = seed;
    std::vector<cv::KeyPoint> k1(n), k2(n + 5);
    for (auto* k : { &k1, &k2 })
        for (size_t i = 0; i < k->size(); i++) { const int level = (int)(rnd() * 4) & 3; (*k)[i].size = 31.0f * std::pow(1.2f, (float)level); (*k)[i].octave = level; }
    Camera c1, c2;
    c1.K.at<float>(0, 0) = 520.f; c1.K.at<float>(1, 1) = 515.f; c1.K.at<float>(0, 2) = 320.5f; c1.K.at<float>(1, 2) = 240.25f;
    c2.K.at<float>(0, 0) = 458.f; c2.K.at<float>(1, 1) = 457.5f; c2.K.at<float>(0, 2) = 367.25f; c2.K.at<float>(1, 2) = 248.5f;
    std::vector<FeatureDescriptor> d1(k1.size()), d2(k2.size());
    W.kf1.reset(new KeyFrame(FeatureViews(k1, d1, FeatureExtractorSettings()), c1));
    W.kf2.reset(new KeyFrame(FeatureViews(k2, d2, FeatureExtractorSettings()), c2));
    W.kf1->SetPose(pose(0.1f, 0.2f, -0.1f, 0.3f));
    W.kf2->SetPose(pose(-0.15f, -0.3f, 0.05f, 0.1f));
    W.lms.clear(); W.matched12.assign(n, nullptr); W.expect_idx1.clear();
    const float a = 0.25f, ca = std::cos(a), sa = std::sin(a);
    for (int i = 0; i < n; i++) {
        const float x = (rnd() - 0.5f) * 4.0f, y = (rnd() - 0.5f) * 3.0f, z = 4.0f + 5.0f * rnd();
        W.lms.emplace_back(new MapPoint()); MapPoint* p1 = W.lms.back().get();
        W.lms.emplace_back(new MapPoint()); MapPoint* p2 = W.lms.back().get();
        p1->mWorldPos.at<float>(0) = x; p1->mWorldPos.at<float>(1) = y; p1->mWorldPos.at<float>(2) = z;
        float bx = scale * (ca * x - sa * y) + 0.4f, by = scale * (sa * x + ca * y) - 0.2f, bz = scale * z + 0.1f;
        if (rnd() < outlier_share) { bx += 1.0f + rnd(); by -= 0.5f + rnd(); }
        p2->mWorldPos.at<float>(0) = bx; p2->mWorldPos.at<float>(1) = by; p2->mWorldPos.at<float>(2) = bz;
        p1->mObservations[W.kf1.get()] = (size_t)i;
        p2->mObservations[W.kf2.get()] = (size_t)((i * 7) % (n + 5));
        bool keep = true;
        if (i % 13 != 4) W.kf1->associateLandMark(i, p1, false); else keep = false;      // a null own point
        if (i % 9 != 2) W.matched12[i] = p2; else keep = false;                          // a null match
        if (i % 17 == 6) { p1->mbBad = true; keep = false; }
        if (i % 19 == 7) { p2->mbBad = true; keep = false; }
        if (i % 23 == 8) { p2->mObservations.clear(); keep = false; }                    // GetIndexInKeyFrame(pKF2) < 0
        if (i % 29 == 9) { p1->mObservations.clear(); keep = false; }                    // GetIndexInKeyFrame(pKF1) < 0
        if (keep) W.expect_idx1.push_back(i);
    }
}

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d (candidate %d, call %d): %s\n", __LINE__, q, call, #c); return 1; } } while (0)

struct Hand { std::vector<hs_sim3_corr> corrs; hs_sim3_params p; hs_sim3_state st; std::vector<uint8_t> best; };

static int same(const HipSim3Solver::Result& r, const World& W, const Hand& H, const hs_sim3_result& res, const std::vector<uint8_t>& inl, int q, int call)
{
    CHECK(std::memcmp(&r.info, &res, sizeof res) == 0);
    CHECK(r.bNoMore == (res.status == HS_SIM3_TOO_FEW || res.status == HS_SIM3_EXHAUSTED));
    const bool found = res.status == HS_SIM3_FOUND;
    CHECK(r.T12.empty() == !found && r.nInliers == res.n_inliers && r.vbInliers.size() == W.matched12.size());
    std::vector<bool> want(W.matched12.size(), false);
    for (size_t k = 0; k < H.corrs.size(); k++) if (inl[k]) want[H.corrs[k].idx1] = true;
    CHECK(want == r.vbInliers);
    if (found) for (int i = 0; i < 16; i++) CHECK(r.T12.at<float>(i / 4, i % 4) == res.T12[i]);
    return 0;
}

int main()
{
    int q = -1, call = -1;
    hs_orb_params op; hs_orb_default_params(&op);
    hs_orb* h = nullptr;
    CHECK(hs_orb_create(&op, 0, &h) == HS_OK);
    const struct { int n; float out, scale; bool fix; int min_inliers; } spec[4] = { { 150, 0.3f, 1.2f, false, 20 }, { 80, 0.2f, 1.0f, true, 15 }, { 12, 0.0f, 1.0f, true, 20 },
                                                                                 { 200, 0.95f, 0.9f, false, 20 } };      // the third: too few
    World W[4]; Hand H[4];
    std::vector<std::unique_ptr<HipSim3Solver>> alone, batch;
    std::vector<HipSim3Solver*> list;
    for (q = 0; q < 4; q++) {
        build(W[q], spec[q].n, spec[q].out, spec[q].scale, 91u + q);
        for (auto* v : { &alone, &batch }) {
            v->emplace_back(new HipSim3Solver(W[q].kf1.get(), W[q].kf2.get(), W[q].matched12, spec[q].fix, 500u + q, h));
            v->back()->SetRansacParameters(0.99, spec[q].min_inliers, 300);
        }
        list.push_back(batch.back().get());
        // the gathering: ascending i1, the skipped entries, and the points in camera frame by hand
        const std::vector<hs_sim3_corr>& g = alone.back()->gathered();
        CHECK(g.size() == W[q].expect_idx1.size() && g.size() < W[q].matched12.size());
        std::vector<MapPoint*> own = W[q].kf1->GetMapPointMatches();
        for (size_t k = 0; k < g.size(); k++) {
            const int i1 = W[q].expect_idx1[k];
            CHECK(g[k].idx1 == i1);
            const cv::Mat T1 = W[q].kf1->GetPose(), X = own[i1]->GetWorldPos();
            for (int r = 0; r < 3; r++) {
                const double v = (((double)T1.at<float>(r, 0) * X.at<float>(0) + (double)T1.at<float>(r, 1) * X.at<float>(1)) + (double)T1.at<float>(r, 2) * X.at<float>(2)) + (double)T1.at<float>(r, 3);
                CHECK(g[k].X1c[r] == (float)v);
            }
            const FeatureExtractorSettings o2 = W[q].kf2->getViews().orbParams();
            const float s2 = W[q].kf2->getViews().keypt((i1 * 7) % (spec[q].n + 5)).size / o2.size_ref;
            CHECK(g[k].sigma2_2 == o2.sigma_ref * (s2 * s2));
        }
        H[q].corrs = g;
        H[q].p = hs_sim3_params{ 0.99, spec[q].min_inliers, 300, spec[q].fix ? 1 : 0, 0, 520.f, 515.f, 320.5f, 240.25f, 458.f, 457.5f, 367.25f, 248.5f, 500u + q };
        hs_sim3_state_init(&H[q].st);
        H[q].best.assign(g.size(), 0);
    }
    int found = 0, too_few = 0;
    for (call = 0; call < 2; call++) {
        std::vector<HipSim3Solver::Result> together;
        HipSim3Solver::iterate(list, 5, together);
        for (q = 0; q < 4; q++) {
            const int64_t off[2] = { 0, (int64_t)H[q].corrs.size() };
            hs_sim3_result res; std::vector<uint8_t> inl(H[q].corrs.size() + 1, 0);
            CHECK(hs_sim3_iterate(h, 1, &H[q].p, off, H[q].corrs.data(), 5, nullptr, 0, &H[q].st, H[q].best.data(), &res, inl.data()) == HS_OK);
            HipSim3Solver::Result one;
            one.T12 = alone[q]->iterate(5, one.bNoMore, one.vbInliers, one.nInliers);
            one.info = together[q].info;                           // (the member call hands back the reference's four values only)
            if (same(together[q], W[q], H[q], res, inl, q, call) || same(one, W[q], H[q], res, inl, q, call)) return 1;
            CHECK(std::memcmp(&alone[q]->state(), &H[q].st, sizeof(hs_sim3_state)) == 0 && std::memcmp(&list[q]->state(), &H[q].st, sizeof(hs_sim3_state)) == 0);
            CHECK(alone[q]->GetEstimatedScale() == H[q].st.s && alone[q]->GetEstimatedRotation().at<float>(1, 2) == H[q].st.R[5] && alone[q]->GetEstimatedTranslation().at<float>(2) == H[q].st.t[2]);
            found += res.status == HS_SIM3_FOUND; too_few += res.status == HS_SIM3_TOO_FEW;
        }
    }
    CHECK(found >= 2 && too_few == 2);
    CHECK(alone[1]->GetEstimatedScale() == 1.0f && std::fabs(alone[0]->GetEstimatedScale() - 1.0f / 1.2f) < 0.02f);      // X1c = s R X2c + t with world B = 1.2 x world A
    std::vector<bool> inl; int n_inl = -1;
    HipSim3Solver fresh(W[3].kf1.get(), W[3].kf2.get(), W[3].matched12, false, 503u, h);
    fresh.SetRansacParameters(0.99, 20, 7);
    const cv::Mat T = fresh.find(inl, n_inl);                      // find = iterate(mRansacMaxIts)
    CHECK(fresh.plan().max_iterations == 7 && fresh.state().iterations >= 1 && fresh.state().iterations <= 7 && (T.empty() ? n_inl == 0 : n_inl > 20) && inl.size() == 200);
    hs_orb_destroy(h);
    std::printf("SIM3 ADAPTOR OK (%d found)\n", found);
    return 0;
}
