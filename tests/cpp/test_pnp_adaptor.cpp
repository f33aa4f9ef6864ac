// HipPnPsolver (hyslam_amd/host/HipPnPsolver.h) on the cv_compat.h stand-ins against the C ABI: the same candidates through the adaptor (Frame,
// FeatureViews, Camera, MapPoint objects, matches with gaps and bad landmarks) and through hs_pnp_iterate on hand-gathered arrays must give identical
// bytes — pose, flag of every keypoint, nInliers, bNoMore — alone, all in one static call, and on a second call (the state persists).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "../../hyslam_amd/host/HipPnPsolver.h"

using namespace HYSLAM;

static uint32_t rng_state;
static float rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (float)((rng_state >> 8) & 0xFFFF) / 65536.0f; }

struct World { std::vector<std::unique_ptr<MapPoint>> lms; std::unique_ptr<Frame> frame; std::vector<MapPoint*> matches; };

// n_kp keypoints; every `gap`-th holds no landmark, every 11th landmark is bad; observations = projections + sub-pixel noise, a share of them wrong
static void build(World& W, int n_kp, int gap, float outlier_share, uint32_t seed)
{
    rng_state = seed;
    const float fx = 520.0f, fy = 515.0f, cx = 320.5f, cy = 240.25f;
    const float a = 0.2f, ca = std::cos(a), sa = std::sin(a);
    const float Rm[3][3] = {{ca, 0, sa}, {0, 1, 0}, {-sa, 0, ca}}, t[3] = {0.3f, -0.2f, 0.4f};
    std::vector<cv::KeyPoint> keys(n_kp);
    W.lms.clear(); W.matches.assign(n_kp, nullptr);
    for (int i = 0; i < n_kp; i++) {
        const float z = 3.0f + 6.0f * rnd(), x = (rnd() - 0.5f) * 4.0f, y = (rnd() - 0.5f) * 3.0f;             // camera frame
        const int level = (int)(rnd() * 8) & 7;
        float du = 0.2f * (rnd() - 0.5f), dv = 0.2f * (rnd() - 0.5f);
        if (rnd() < outlier_share) { du += 40.0f + 60.0f * rnd(); dv -= 30.0f + 50.0f * rnd(); }
        keys[i].pt.x = fx * x / z + cx + du; keys[i].pt.y = fy * y / z + cy + dv; keys[i].size = 31.0f * std::pow(1.2f, (float)level); keys[i].octave = level;
        if (gap && i % gap == 1) continue;
        W.lms.emplace_back(new MapPoint());
        MapPoint* lm = W.lms.back().get();
        const float pc[3] = {x - t[0], y - t[1], z - t[2]};                                                    // Xw = R^T (Pc - t)
        for (int r = 0; r < 3; r++) lm->mWorldPos.at<float>(r) = Rm[0][r] * pc[0] + Rm[1][r] * pc[1] + Rm[2][r] * pc[2];
        lm->mbBad = i % 11 == 5;
        W.matches[i] = lm;
    }
    Camera cam; cam.sensor = 0;
    cam.K.at<float>(0, 0) = fx; cam.K.at<float>(1, 1) = fy; cam.K.at<float>(0, 2) = cx; cam.K.at<float>(1, 2) = cy;
    std::vector<FeatureDescriptor> d(n_kp);
    W.frame.reset(new Frame(FeatureViews(keys, d, FeatureExtractorSettings()), cam));
}

// the same candidate by hand: the correspondences in keypoint order, then the C ABI
struct Hand { std::vector<hs_pnp_corr> corrs; hs_pnp_params p; hs_pnp_state st; std::vector<uint8_t> best; };
static void gather(const World& W, uint64_t seed, Hand& H)
{
    const FeatureViews& views = W.frame->getViews();
    const FeatureExtractorSettings orb = views.orbParams();
    H.corrs.clear();
    for (size_t i = 0; i < W.matches.size(); i++) {
        MapPoint* mp = W.matches[i];
        if (!mp || mp->isBad()) continue;
        const cv::KeyPoint kp = views.keypt(i);
        const cv::Mat X = mp->GetWorldPos();
        const float s = kp.size / orb.size_ref;
        H.corrs.push_back(hs_pnp_corr{ { X.at<float>(0), X.at<float>(1), X.at<float>(2) }, kp.pt.x, kp.pt.y, orb.sigma_ref * (s * s), (int32_t)i, 0 });
    }
    const Camera& c = W.frame->getCamera();
    H.p = hs_pnp_params{ 0.99, 10, 12, 4, 0.5f, 5.991f, c.fx(), c.fy(), c.cx(), c.cy(), 0, seed };
    hs_pnp_state_init(&H.st);
    H.best.assign(H.corrs.size(), 0);
}

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d (candidate %d, call %d): %s\n", __LINE__, q, call, #c); return 1; } } while (0)

static int same(const HipPnPsolver::Result& r, const World& W, const Hand& H, const hs_pnp_result& res, const std::vector<uint8_t>& inl, int q, int call)
{
    CHECK(std::memcmp(&r.info, &res, sizeof res) == 0);
    CHECK(r.bNoMore == (res.status != HS_PNP_REFINED));
    const bool pose = res.status == HS_PNP_REFINED || res.status == HS_PNP_BEST;
    CHECK(r.Tcw.empty() == !pose && r.nInliers == (pose ? res.n_inliers : 0) && r.vbInliers.size() == (pose ? W.matches.size() : 0));
    if (!pose) return 0;
    std::vector<bool> want(W.matches.size(), false);
    for (size_t k = 0; k < H.corrs.size(); k++) if (inl[k]) want[H.corrs[k].kp] = true;
    CHECK(want == r.vbInliers);
    for (int i = 0; i < 16; i++) CHECK(r.Tcw.at<float>(i / 4, i % 4) == res.Tcw[i]);
    return 0;
}

int main()
{
    int q = -1, call = -1;
    hs_orb_params op; hs_orb_default_params(&op);
    hs_orb* h = nullptr;
    CHECK(hs_orb_create(&op, 0, &h) == HS_OK);
    const struct { int n, gap; float out; } spec[4] = { { 120, 7, 0.25f }, { 65, 0, 0.3f }, { 11, 3, 0.0f }, { 300, 5, 0.9f } };   // the third: too few
    World W[4]; Hand H[4];
    std::vector<std::unique_ptr<HipPnPsolver>> alone, batch;
    std::vector<HipPnPsolver*> list;
    for (q = 0; q < 4; q++) {
        build(W[q], spec[q].n, spec[q].gap, spec[q].out, 77u + q);
        gather(W[q], 1000u + q, H[q]);
        for (auto* v : { &alone, &batch }) {
            v->emplace_back(new HipPnPsolver(*W[q].frame, W[q].matches, 1000u + q, h));
            v->back()->SetRansacParameters(0.99, 10, 12, 4, 0.5f, 5.991f);
        }
        list.push_back(batch.back().get());
        CHECK(alone.back()->correspondences() == (int)H[q].corrs.size());
    }
    int refined = 0, too_few = 0;
    for (call = 0; call < 2; call++) {
        std::vector<HipPnPsolver::Result> together;
        HipPnPsolver::iterate(list, call ? 3 : 12, together);
        for (q = 0; q < 4; q++) {
            const int64_t off[2] = { 0, (int64_t)H[q].corrs.size() };
            hs_pnp_result res; std::vector<uint8_t> inl(H[q].corrs.size(), 0);
            CHECK(hs_pnp_iterate(h, 1, &H[q].p, off, H[q].corrs.data(), call ? 3 : 12, nullptr, 0, &H[q].st, H[q].best.data(), &res, inl.data()) == HS_OK);
            HipPnPsolver::Result one;
            one.Tcw = alone[q]->iterate(call ? 3 : 12, one.bNoMore, one.vbInliers, one.nInliers);
            one.info = together[q].info;                           // (the member call hands back the reference's four values only)
            if (same(together[q], W[q], H[q], res, inl, q, call) || same(one, W[q], H[q], res, inl, q, call)) return 1;
            CHECK(std::memcmp(&alone[q]->state(), &H[q].st, sizeof(hs_pnp_state)) == 0 && std::memcmp(&list[q]->state(), &H[q].st, sizeof(hs_pnp_state)) == 0);
            refined += res.status == HS_PNP_REFINED; too_few += res.status == HS_PNP_TOO_FEW;
        }
    }
    CHECK(refined >= 2 && too_few == 2);
    std::vector<bool> inl; int n_inl = -1;
    HipPnPsolver fresh(*W[0].frame, W[0].matches, 1000u, h);
    fresh.SetRansacParameters(0.99, 10, 12, 4, 0.5f, 5.991f);
    const cv::Mat T = fresh.find(inl, n_inl);                      // find = iterate(mRansacMaxIts)
    CHECK(fresh.plan().max_iterations == 12 && fresh.state().iterations >= 1 && fresh.state().iterations <= 12 && (T.empty() || n_inl > fresh.plan().min_inliers - 1));
    hs_orb_destroy(h);
    std::printf("PNP ADAPTOR OK (%d refined)\n", refined);
    return 0;
}
