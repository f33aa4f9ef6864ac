// HipPoseOptimizer::PoseOptimization (hyslam_amd/host/HipPoseOptimizer.h) on the cv_compat.h stand-ins against the C ABI: the same problem through
// the adaptor (Frame, FeatureViews, Camera, MapPoint objects) and through hs_pose_optimize on hand-gathered arrays must give identical bytes — pose,
// flag of every keypoint, return value.  Frames: stereo with gaps in the associations and gross outliers, monocular, fewer than 10 edges (one round),
// fewer than 3 edges (nothing runs: pose and return value as the reference leaves them).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "../../hyslam_amd/host/HipPoseOptimizer.h"

using namespace HYSLAM;

static uint32_t rng_state;
static float rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (float)((rng_state >> 8) & 0xFFFF) / 65536.0f; }
static float gauss() { float s = 0; for (int i = 0; i < 12; i++) s += rnd(); return s - 6.0f; }

struct World { std::vector<std::unique_ptr<MapPoint>> lms; std::unique_ptr<Frame> frame; std::vector<int> held; };

// n_kp keypoints, every `gap`-th without a landmark; pose = a small rotation about y and a translation; observations = projections + noise
static void build(World& W, int n_kp, int gap, bool stereo, float outlier_share, uint32_t seed)
{
    rng_state = seed;
    const float fx = 700.0f, fy = 700.0f, cx = 640.0f, cy = 360.0f, bf = 84.0f;
    const float a = 0.03f, ca = std::cos(a), sa = std::sin(a);
    const float Rm[3][3] = {{ca, 0, sa}, {0, 1, 0}, {-sa, 0, ca}}, t[3] = {0.1f, -0.05f, 0.2f};
    std::vector<cv::KeyPoint> keys(n_kp);
    std::vector<float> uR(n_kp, -1.0f), depth(n_kp, -1.0f);
    W.lms.clear(); W.held.clear();
    std::vector<MapPoint*> of_kp(n_kp, nullptr);
    for (int i = 0; i < n_kp; i++) {
        const float z = 2.0f + 23.0f * rnd(), x = (rnd() - 0.5f) * 1.6f * z, y = (rnd() - 0.5f) * 0.9f * z;      // camera frame
        const int level = (int)(rnd() * 8) & 7;
        const float s = std::pow(1.2f, (float)level);
        float du = 0.6f * s * gauss(), dv = 0.6f * s * gauss();
        if (rnd() < outlier_share) { du += 40.0f + 60.0f * rnd(); dv -= 30.0f + 50.0f * rnd(); }
        keys[i].pt.x = fx * x / z + cx + du; keys[i].pt.y = fy * y / z + cy + dv; keys[i].size = 31.0f * s; keys[i].octave = level;
        if (stereo && i % 5 != 2) { uR[i] = std::fmax(0.0f, keys[i].pt.x - bf / z + 0.5f * s * gauss()); depth[i] = z; }
        if (gap && i % gap == 1) continue;
        W.lms.emplace_back(new MapPoint());
        MapPoint* lm = W.lms.back().get();
        const float pc[3] = {x - t[0], y - t[1], z - t[2]};                                                    // Xw = R^T (Pc - t)
        for (int r = 0; r < 3; r++) lm->mWorldPos.at<float>(r) = Rm[0][r] * pc[0] + Rm[1][r] * pc[1] + Rm[2][r] * pc[2];
        of_kp[i] = lm;
    }
    Camera cam; cam.sensor = stereo ? 1 : 0; cam.mbf = bf;
    cam.K.at<float>(0, 0) = fx; cam.K.at<float>(1, 1) = fy; cam.K.at<float>(0, 2) = cx; cam.K.at<float>(1, 2) = cy;
    std::vector<FeatureDescriptor> d(n_kp);
    FeatureExtractorSettings orb;
    W.frame.reset(stereo ? new Frame(FeatureViews(keys, keys, uR, depth, d, d, orb), cam) : new Frame(FeatureViews(keys, d, orb), cam));
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) T.at<float>(r, c) = r == c ? 1.0f : 0.0f;
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) T.at<float>(r, c) = Rm[r][c]; T.at<float>(r, 3) = t[r] + 0.02f * (float)(r - 1); }   // a start a few cm off
    W.frame->SetPose(T);
    for (int i = 0; i < n_kp; i++) if (of_kp[i]) { W.frame->associateLandMark(i, of_kp[i], true); W.held.push_back(i); }
}

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d (case %d): %s\n", __LINE__, which, #c); return 1; } } while (0)

int main()
{
    hs_orb_params prm; hs_orb_default_params(&prm);
    hs_orb* h = nullptr;
    if (hs_orb_create(&prm, 0, &h) != HS_OK) { std::printf("FAILED: no handle\n"); return 1; }
    struct Case { int n_kp, gap; bool stereo; float share; } cases[] = {
        {400, 7, true, 0.15f}, {257, 0, true, 0.3f}, {120, 3, false, 0.15f}, {9, 0, true, 0.0f}, {12, 2, true, 0.0f}, {2, 0, true, 0.0f}, {4, 2, false, 0.0f}, {0, 0, true, 0.0f}};
    int ran = 0, skipped = 0, bad_total = 0;
    for (int which = 0; which < (int)(sizeof(cases) / sizeof(cases[0])); which++) {
        const Case& c = cases[which];
        World W;
        build(W, c.n_kp, c.gap, c.stereo, c.share, 1234u + 77u * (uint32_t)which);
        Frame* F = W.frame.get();
        // the problem by hand, from the same objects, BEFORE the adaptor changes the frame
        std::vector<hs_pose_edge> edges;
        for (int i : W.held) {
            hs_pose_edge e;
            MapPoint* lm = F->hasAssociation(i);
            for (int k = 0; k < 3; k++) e.Xw[k] = lm->mWorldPos.at<float>(k);
            const cv::KeyPoint kp = F->getViews().keypt(i);
            e.u = kp.pt.x; e.v = kp.pt.y; e.ur = F->getViews().uR(i);
            const float sf = kp.size / 31.0f;
            e.inv_sigma2 = 1 / (1.0f * (sf * sf));
            e.kp = i;
            edges.push_back(e);
        }
        hs_pose_problem P;
        for (int r = 0; r < 4; r++) for (int k = 0; k < 4; k++) P.Tcw[4 * r + k] = F->mTcw.at<float>(r, k);
        P.fx = 700.0f; P.fy = 700.0f; P.cx = 640.0f; P.cy = 360.0f; P.bf = 84.0f;
        const int64_t off[2] = {0, (int64_t)edges.size()};
        std::vector<uint8_t> flags(edges.size() + 1, 0x55);
        hs_pose_result R;
        std::memset(&R, 0x55, sizeof(R));
        CHECK(hs_pose_optimize(h, 1, &P, off, edges.data(), flags.data(), &R) == HS_OK);
        CHECK(flags[edges.size()] == 0x55);
        for (int i : W.held) F->setOutlier(i, true);                       // the adaptor resets every flag while it gathers, as the reference does
        HipPoseOptimizer::Info info;
        const int n_good = HipPoseOptimizer::PoseOptimization(F, optInfo(), h, &info);
        CHECK(info.n_edges == (int)edges.size() && R.n_edges == (int)edges.size());
        if (edges.size() < 3) {
            CHECK(n_good == 0 && R.n_good == 0 && R.status == HS_POSE_TOO_FEW && info.status == HS_POSE_TOO_FEW);
            for (int r = 0; r < 4; r++) for (int k = 0; k < 4; k++) CHECK(F->mTcw.at<float>(r, k) == P.Tcw[4 * r + k] && R.Tcw[4 * r + k] == P.Tcw[4 * r + k]);
            for (size_t k = 0; k < edges.size(); k++) CHECK(flags[k] == 0x55 && !F->isOutlier(edges[k].kp));
            skipped++;
            continue;
        }
        CHECK(R.status == HS_POSE_OK && info.status == HS_POSE_OK && n_good == R.n_good && info.rounds == R.rounds && R.rounds == (edges.size() < 10 ? 1 : 4));
        CHECK(info.lm_iterations == R.lm_iterations && info.lm_trials == R.lm_trials);
        for (int r = 0; r < 4; r++) for (int k = 0; k < 4; k++) CHECK(std::memcmp(&F->mTcw.at<float>(r, k), &R.Tcw[4 * r + k], 4) == 0);
        int bad = 0;
        for (size_t k = 0; k < edges.size(); k++) { CHECK(flags[k] <= 1 && F->isOutlier(edges[k].kp) == (flags[k] != 0)); bad += flags[k]; }
        CHECK(n_good == (int)edges.size() - bad);
        if (c.share > 0.12f) CHECK(bad > 0 && bad < (int)edges.size() / 2);   // the gross outliers are found, the rest kept
        // the start is 2 cm off the truth in x and in z.  With n edges of pixel noise s at depth z the translation is known to about z s / (fx sqrt(n)):
        // 12 * 1.3 / 700 / sqrt(50) = 3 mm for 50 edges, so there the result is closer to the truth than the start in both components; with the 9 and
        // 6 edges of the small cases that figure is the size of the start offset itself (about 1 to 2 cm) and nothing is claimed
        if (edges.size() >= 50) CHECK(std::fabs(F->mTcw.at<float>(0, 3) - 0.1f) < 0.02f && std::fabs(F->mTcw.at<float>(2, 3) - 0.2f) < 0.02f);
        bad_total += bad;
        ran++;
    }
    hs_orb_destroy(h);
    if (ran != 5 || skipped != 3 || bad_total == 0) { std::printf("FAILED: %d ran, %d skipped, %d outliers\n", ran, skipped, bad_total); return 1; }
    std::printf("POSE OPTIMIZER ADAPTOR OK (%d optimised, %d below three edges, %d outliers)\n", ran, skipped, bad_total);
    return 0;
}
