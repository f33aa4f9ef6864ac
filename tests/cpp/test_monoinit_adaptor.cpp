// HipMonoEstimator (hyslam_amd/host/HipMonoEstimator.h) on the cv_compat.h stand-ins against the C ABI: the same two-view problems through the adaptor
// (Frame, FeatureViews, Camera objects; matches with -1 entries; n1 != n2) and through hs_monoinit_estimate on hand-gathered arrays must give
// identical bytes — the record, R21, t21, every point and flag — alone, all in one static call, and on a second call (there is no state).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "../../hyslam_amd/host/HipMonoEstimator.h"

using namespace HYSLAM;

static uint32_t rng_state;
static float rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (float)((rng_state >> 8) & 0xFFFF) / 65536.0f; }

struct World { std::unique_ptr<Frame> f1, f2; std::vector<int> m12; std::vector<hs_keypoint> k1, k2; };

static hs_keypoint key_of(const cv::KeyPoint& k) { hs_keypoint o = hs_keypoint(); o.x = k.pt.x; o.y = k.pt.y; o.size = k.size; o.angle = k.angle; o.response = k.response; o.octave = k.octave; return o; }

// n matched points of a scene (a plane, or depths 3 .. 9) seen from two cameras, `extra` unmatched key points in each frame, frame 2 reversed
static void build(World& W, int n, bool plane, bool moved, uint32_t seed)
{
    rng_state = seed;
    const int n1 = n + n / 3 + 2, n2 = n + n / 2 + 5;
    std::vector<cv::KeyPoint> k1(n1), k2(n2);
    for (auto* k : { &k1, &k2 }) for (auto& kp : *k) { kp.pt.x = rnd() * 640.f; kp.pt.y = rnd() * 480.f; kp.size = 31.f; }
    W.m12.assign(n1, -1);
    const float a = 0.05f, ca = std::cos(a), sa = std::sin(a);
    for (int i = 0; i < n; i++) {
        const float u = rnd() - 0.5f, v = (rnd() - 0.5f) * 0.75f;
        const float z = plane ? 5.0f / (1.0f - 0.16f * u - 0.1f * v) : 3.0f + 6.0f * rnd();
        const float X = u * z, Y = v * z;
        const float X2 = ca * X + sa * z + (moved ? 0.4f : 0.f), Y2 = Y + (moved ? 0.05f : 0.f), Z2 = -sa * X + ca * z + (moved ? 0.1f : 0.f);
        const int i1 = i + i / 3, i2 = n2 - 1 - (i + i / 2);
        k1[i1].pt.x = 500.f * X / z + 320.f + (rnd() - 0.5f) * 0.4f; k1[i1].pt.y = 500.f * Y / z + 240.f + (rnd() - 0.5f) * 0.4f;
        k2[i2].pt.x = 500.f * X2 / Z2 + 320.f + (rnd() - 0.5f) * 0.4f; k2[i2].pt.y = 500.f * Y2 / Z2 + 240.f + (rnd() - 0.5f) * 0.4f;
        W.m12[i1] = i2;
    }
    Camera c;
    c.K.at<float>(0, 0) = 500.f; c.K.at<float>(1, 1) = 500.f; c.K.at<float>(0, 2) = 320.f; c.K.at<float>(1, 2) = 240.f; c.K.at<float>(2, 2) = 1.f;
    std::vector<FeatureDescriptor> d1(k1.size()), d2(k2.size());
    W.f1.reset(new Frame(FeatureViews(k1, d1, FeatureExtractorSettings()), c));
    W.f2.reset(new Frame(FeatureViews(k2, d2, FeatureExtractorSettings()), c));
    W.k1.clear(); W.k2.clear();
    for (auto& k : k1) W.k1.push_back(key_of(k));
    for (auto& k : k2) W.k2.push_back(key_of(k));
}

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d (problem %d, call %d): %s\n", __LINE__, q, call, #c); return 1; } } while (0)

int main()
{
    int q = -1, call = -1;
    hs_orb_params op; hs_orb_default_params(&op);
    hs_orb* h = nullptr;
    CHECK(hs_orb_create(&op, 0, &h) == HS_OK);
    const struct { int n; bool plane, moved; } spec[4] = { { 150, false, true }, { 150, true, true }, { 7, false, true }, { 120, false, false } };   // the third: too few; the fourth: no parallax
    World W[4];
    std::vector<std::unique_ptr<HipMonoEstimator>> alone, batch;
    std::vector<HipMonoEstimator*> list; std::vector<const Frame*> frames; std::vector<const std::vector<int>*> matches;
    MonoEstimatorParams mp; mp.sigma = 1.0f; mp.MaxIterations = 60; mp.minTriangulated = 50; mp.minFracTriangulated = 0.9f;
    for (q = 0; q < 4; q++) {
        build(W[q], spec[q].n, spec[q].plane, spec[q].moved, 91u + q);
        alone.emplace_back(new HipMonoEstimator(*W[q].f1, mp, 500u + q, h));
        batch.emplace_back(new HipMonoEstimator(*W[q].f1, mp, 500u + q, h));
        list.push_back(batch.back().get()); frames.push_back(W[q].f2.get()); matches.push_back(&W[q].m12);
        CHECK(alone.back()->keys().size() == W[q].k1.size() && std::memcmp(alone.back()->keys().data(), W[q].k1.data(), W[q].k1.size() * sizeof(hs_keypoint)) == 0);
        CHECK(W[q].k1.size() != W[q].k2.size());
    }
    int ok_h = 0, ok_f = 0, too_few = 0, failed = 0;
    for (call = 0; call < 2; call++) {
        std::vector<HipMonoEstimator::Result> together;
        HipMonoEstimator::Initialize(list, frames, matches, together);
        for (q = 0; q < 4; q++) {
            const size_t n1 = W[q].k1.size();
            const int64_t off1[2] = { 0, (int64_t)n1 }, off2[2] = { 0, (int64_t)W[q].k2.size() };
            hs_monoinit_params p = hs_monoinit_params{ 500.f, 500.f, 320.f, 240.f, 1.0f, 60, 50, 0.9f, 1.0f, 0, 500u + q };
            CHECK(std::memcmp(&p, &alone[q]->params(), sizeof p) == 0);
            hs_monoinit_result res; std::vector<uint8_t> ih(n1), jf(n1), tri(n1); std::vector<float> p3d(3 * n1);
            std::vector<int32_t> m(W[q].m12.begin(), W[q].m12.end());
            CHECK(hs_monoinit_estimate(h, 1, &p, off1, W[q].k1.data(), off2, W[q].k2.data(), m.data(), nullptr, 0, &res, ih.data(), jf.data(), p3d.data(), tri.data()) == HS_OK);
            const HipMonoEstimator::Result& r = together[q];
            const bool ok = res.status == HS_MONOINIT_OK_H || res.status == HS_MONOINIT_OK_F;
            CHECK(std::memcmp(&r.info, &res, sizeof res) == 0 && r.ok == ok && r.R21.empty() == !ok && r.t21.empty() == !ok);
            CHECK(r.vP3D.size() == n1 && r.vbTriangulated.size() == n1 && r.inliers_h == ih && r.inliers_f == jf);
            for (size_t i = 0; i < n1; i++)
                CHECK(r.vbTriangulated[i] == (tri[i] != 0) && std::memcmp(&r.vP3D[i].x, &p3d[3 * i], 4) == 0 && std::memcmp(&r.vP3D[i].y, &p3d[3 * i + 1], 4) == 0 &&
                      std::memcmp(&r.vP3D[i].z, &p3d[3 * i + 2], 4) == 0);
            // the member form: the reference's signature; outputs untouched where it returns false
            cv::Mat R21, t21; std::vector<cv::Point3f> vP3D(3, cv::Point3f(1.f, 2.f, 3.f)); std::vector<bool> vbT(2, true);
            const bool got = alone[q]->Initialize(*W[q].f2, W[q].m12, R21, t21, vP3D, vbT);
            CHECK(got == ok);
            if (ok) {
                for (int i = 0; i < 9; i++) CHECK(R21.at<float>(i / 3, i % 3) == res.R21[i] && r.R21.at<float>(i / 3, i % 3) == res.R21[i]);
                for (int i = 0; i < 3; i++) CHECK(t21.at<float>(i) == res.t21[i] && r.t21.at<float>(i) == res.t21[i]);
                CHECK(vP3D.size() == n1 && vbT == r.vbTriangulated && res.n_triangulated > 50);
                const double deg = HipMonoEstimator::parallax_deg(res);
                CHECK(deg >= 1.0 && deg < 20.0);
            } else
                CHECK(R21.empty() && t21.empty() && vP3D.size() == 3 && vP3D[2].z == 3.f && vbT.size() == 2);
            ok_h += res.status == HS_MONOINIT_OK_H; ok_f += res.status == HS_MONOINIT_OK_F; too_few += res.status == HS_MONOINIT_TOO_FEW; failed += res.status == HS_MONOINIT_FAILED;
        }
    }
    CHECK(ok_f == 2 && ok_h == 2 && too_few == 2 && failed == 2);
    hs_orb_destroy(h);
    std::printf("MONOINIT ADAPTOR OK (%d by F, %d by H)\n", ok_f, ok_h);
    return 0;
}
