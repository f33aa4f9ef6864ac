// HipKeyFrameGraph::localMap (hyslam_amd/host/HipKeyFrameGraph.h) on the cv_compat.h stand-ins against a literal walk written from
// TrackLocalMap::UpdateLocalKeyFrames, UpdateLocalPoints and the head of SearchLocalPoints (src/slam/tracking/TrackLocalMap.cpp:55-67,80-184): the
// std::set<KeyFrame*> iterated while it grows, each local key frame's GetMapPointMatches(), the erase of what the frame already holds.  The world
// is a map of 48 key frames that see 2 000 landmarks in runs of up to 8 consecutive key frames.  Frames, spanning trees and parameters are varied so
// that the walk ends in each of its ways.
#include <cstdio>
#include <cstdlib>
#include "../../hyslam_amd/host/HipKeyFrameGraph.h"
#include "localmap_restatement.h"

static uint32_t rng_state;
static uint32_t rnd(uint32_t n) { rng_state = rng_state * 1664525u + 1013904223u; return (rng_state >> 8) % n; }

static void build(MapWorld& W, int n_kf, int n_lm)
{
    rng_state = 4242;
    std::vector<std::vector<cv::KeyPoint>> keys(n_kf);
    std::vector<std::vector<std::pair<int, int>>> assoc(n_kf);
    for (int lm = 0; lm < n_lm; lm++) {
        const int n = lm % 50 == 7 ? 0 : 1 + (int)rnd(8), first = (int)rnd((uint32_t)(n_kf - n + 1));     // every 50th landmark has no observer
        for (int kf = first; kf < first + n; kf++) {
            keys[kf].push_back(cv::KeyPoint());
            if (keys[kf].size() % 4 == 0) keys[kf].push_back(cv::KeyPoint());                            // a key point without a landmark
            assoc[kf].push_back({(int)keys[kf].size() - 1, lm});
        }
    }
    for (int i = 0; i < n_lm; i++) W.lms.emplace_back(new MapPoint());
    for (int kf = 0; kf < n_kf; kf++) {
        Camera cam; cam.sensor = 1;
        std::vector<FeatureDescriptor> d(keys[kf].size());
        const std::vector<float> none(keys[kf].size(), -1.0f);
        W.kfs.emplace_back(new KeyFrame(FeatureViews(keys[kf], keys[kf], none, none, d, d, FeatureExtractorSettings()), cam));
        KeyFrame* p = W.kfs.back().get();
        p->mnId = (unsigned long)kf;
        for (const auto& va : assoc[kf]) {
            MapPoint* lm = W.lms[va.second].get();
            p->associateLandMark(va.first, lm, true);
            lm->mObservations[p] = (size_t)va.first;
            lm->nObs++;
        }
    }
    for (int i = 3; i < n_lm; i += 13) W.lms[i]->mbBad = true;
    for (auto& k : W.kfs) {
        std::map<KeyFrame*, int> counter; std::vector<int> ws;
        ref_update_connections(W, k.get(), 3, counter, W.ordered[k.get()], ws);
    }
    for (int kf = 2; kf < n_kf; kf += 5) W.kfs[kf]->mbBad = true;         // after the lists were made: they still name these key frames
}

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d (case %d): %s\n", __LINE__, which, #c); return 1; } } while (0)

int main()
{
    const int n_kf = 48, n_lm = 2000;
    MapWorld W;
    build(W, n_kf, n_lm);
    HipKeyFrameGraph g;
    int grew = 0, by_parent = 0, by_limit = 0, walked_out = 0, removed = 0, selected = 0;
    for (int which = 0; which < 24; which++) {
        // spanning tree: everyone hangs on its predecessor (the usual map), only every seventh key frame has a parent, or nobody has
        for (int kf = 0; kf < n_kf; kf++) {
            KeyFrame* par = kf > 0 ? W.kfs[kf - 1].get() : nullptr;
            W.kfs[kf]->mpParent = which % 3 == 0 ? par : (which % 3 == 1 && kf % 7 == 3 ? W.kfs[(kf * 5 + 11) % n_kf].get() : nullptr);
        }
        TrackLocalMapParameters params;
        static const int n_max[6] = {80, 80, 80, 6, 12, 0}, n_neighbor[4] = {10, 3, 0, 1};
        params.N_max_local_keyframes = n_max[which % 6];
        params.N_neighbor_keyframes = n_neighbor[which % 4];
        // the frame holds 150 landmarks seen around key frame `centre` (bad ones among them), or nothing
        rng_state = 99u + (uint32_t)which;
        Frame F;
        const int centre = (int)rnd((uint32_t)n_kf);
        int view = 0;
        for (int tries = 0; tries < 4000 && view < (which == 23 ? 0 : 150); tries++) {
            MapPoint* pMP = W.lms[rnd((uint32_t)n_lm)].get();
            bool near = pMP->mObservations.empty() && tries % 9 == 0;
            for (const auto& ob : pMP->mObservations) near = near || std::abs((int)ob.first->mnId - centre) <= 3;
            if (near && F.associateLandMark(view * 2 + 1, pMP, true) == 0) view++;
        }
        const Literal want = literal(F, &W, params);
        const HipKeyFrameGraph::LocalMap got = g.localMap(F, &W, params);
        CHECK(got.key_frames == want.local_key_frames);
        CHECK(got.map_points == want.v_lmp);
        CHECK(got.bad_matches == want.removed);
        std::map<KeyFrame*, int> counter; int mx = 0; KeyFrame* kmax = nullptr;
        std::vector<MapPoint*> held;
        for (const auto& kv : F.getLandMarkMatches()) held.push_back(kv.second);
        ref_local_votes(held, counter, kmax, mx);
        CHECK(got.max_kf == kmax && got.max_count == mx);
        size_t first = 0;
        for (const auto& kc : counter) first += !kc.first->isBad();
        bool parent_in = false;
        for (KeyFrame* p : want.local_key_frames) parent_in = parent_in || p->GetParent();
        grew += want.local_key_frames.size() > first;
        by_parent += parent_in;
        by_limit += first > 0 && want.local_key_frames.size() > (size_t)params.N_max_local_keyframes;
        walked_out += first > 0 && !parent_in && want.local_key_frames.size() <= (size_t)params.N_max_local_keyframes;
        removed += (int)want.removed.size();
        selected += (int)want.v_lmp.size();
        if (which == 23) CHECK(want.local_key_frames.empty() && want.v_lmp.empty());
    }
    const int which = -1;
    CHECK(grew > 5 && by_parent > 5 && by_limit > 2 && walked_out > 2 && removed > 20 && selected > 2000);
    std::printf("grew %d, ended on a parent %d, on the limit %d, walked out %d; %d associations removed, %d landmarks selected\nLOCAL MAP ADAPTOR OK\n",
                grew, by_parent, by_limit, walked_out, removed, selected);
    return 0;
}
