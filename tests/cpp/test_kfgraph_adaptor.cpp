// hyslam_amd/host/HipKeyFrameGraph.h on the cv_compat.h stand-ins against a plain std::map restatement of CovisNode::UpdateConnections
// (src/core/CovisibilityGraph.cpp:42-124), TrackLocalMap::UpdateLocalKeyFrames (src/slam/tracking/TrackLocalMap.cpp:80-123) and KeyFrameCuller::run
// (src/slam/mapping/KeyFrameCuller.cpp:21-93).  Two identical worlds are built: the restatement culls in one, the adaptor in the other.  The world holds
// two groups of 40 landmarks, one seen by exactly the key frames 1-4 and one by exactly 6-10, and those key frames hold at most three other landmarks:
// on the first snapshot all nine are redundant.  In the sequence, culling key frame 1 takes the first group down to Observations() == thObs, so 2-4 are
// kept; 6 and 7 go before the second group gets there, 8-10 are kept.  The other key frames share 900 random landmarks.
#include <cstdio>
#include "../../hyslam_amd/host/HipKeyFrameGraph.h"
#include "kfgraph_restatement.h"

static uint32_t rng_state;
static uint32_t rnd(uint32_t n) { rng_state = rng_state * 1664525u + 1013904223u; return (rng_state >> 8) % n; }

static void build(World& W, int n_kf, int n_random, int views_per_kf)
{
    rng_state = 12345;
    std::vector<std::vector<cv::KeyPoint>> keys(n_kf);
    std::vector<std::vector<float>> depth(n_kf);
    std::vector<std::vector<std::pair<int, int>>> assoc(n_kf);            // (view, landmark)
    const auto observe = [&](int kf, int lm, int octave, float d) {
        cv::KeyPoint kp; kp.octave = octave;
        keys[kf].push_back(kp); depth[kf].push_back(d);
        assoc[kf].push_back({(int)keys[kf].size() - 1, lm});
    };
    int n_lm = 0;
    for (int i = 0; i < 40; i++, n_lm++) for (int kf = 1; kf <= 4; kf++) observe(kf, n_lm, 1, 5.0f);       // the group of four
    for (int i = 0; i < 40; i++, n_lm++) for (int kf = 6; kf <= 10; kf++) observe(kf, n_lm, 2, 7.0f);      // the group of five
    const int n_group = n_lm;
    const auto room = [&](int kf) { return (kf >= 1 && kf <= 4) || (kf >= 6 && kf <= 10) ? 43 : views_per_kf; };   // 40 of 43 is above frac_redundant
    for (int i = 0; i < n_random; i++, n_lm++) {
        const int n = 1 + (int)rnd(7);
        std::set<int> who;
        while ((int)who.size() < n) who.insert((int)rnd(n_kf));
        for (int kf : who) if ((int)keys[kf].size() < room(kf)) observe(kf, n_lm, (int)rnd(8), (float)rnd(60) - 3.0f);
    }
    for (int i = 0; i < n_lm; i++) W.lms.emplace_back(new MapPoint());
    for (int kf = 0; kf < n_kf; kf++) {
        Camera cam; cam.sensor = 1;
        std::vector<FeatureDescriptor> d(keys[kf].size());
        W.kfs.emplace_back(new KeyFrame(FeatureViews(keys[kf], keys[kf], std::vector<float>(keys[kf].size(), -1.0f), depth[kf], d, d, FeatureExtractorSettings()), cam));
        KeyFrame* p = W.kfs.back().get();
        p->mnId = (unsigned long)kf; p->mThDepth = 35.0f;
        for (const auto& va : assoc[kf]) {
            MapPoint* lm = W.lms[va.second].get();
            p->associateLandMark(va.first, lm, true);
            lm->mObservations[p] = (size_t)va.first;
            lm->nObs += (va.second % 5 == 0 && va.second >= n_group) ? 2 : 1;                                 // a stereo observation counts twice
        }
    }
    for (int i = n_group + 5; i < n_lm; i += 17) W.lms[i]->mbBad = true;
    W.kfs[n_kf - 1]->mbBad = true;
    W.kfs[n_kf - 2]->mnId = 3;                                                                           // an id carried twice
    for (int kf = 0; kf < n_kf - 1; kf++) W.covisible.push_back(W.kfs[kf].get());                        // key frame 0 is among them: skipped (:31)
}

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main()
{
    const int n_kf = 14;
    World A, B;
    build(A, n_kf, 900, 400);
    build(B, n_kf, 900, 400);
    HipKeyFrameGraph g;

    // UpdateConnections for every key frame, at the reference's threshold and at small ones (longer lists, ties)
    for (int th : {15, 4, 1}) {
        for (int k = 0; k < n_kf; k++) {
            std::map<KeyFrame*, int> counter; std::vector<KeyFrame*> ordered; std::vector<int> ws;
            ref_update_connections(A, A.kfs[k].get(), th, counter, ordered, ws);
            const HipKeyFrameGraph::Connections c = g.updateConnections(A.kfs[k].get(), th);
            CHECK(c.weights == counter);
            CHECK(c.ordered == ordered && c.ordered_weights == ws);
            CHECK(c.symmetric_updates.size() == ordered.size());
            for (size_t i = 0; i < ordered.size(); i++) CHECK(c.symmetric_updates.at(ordered[i]) == ws[i]);
        }
    }

    // UpdateLocalKeyFrames: a frame matched to every third landmark
    {
        Frame F;
        std::vector<MapPoint*> matched;
        int view = 0, n_bad = 0;
        for (size_t i = 0; i < A.lms.size(); i += 3) {
            MapPoint* pMP = A.lms[i].get();
            F.associateLandMark(view++, pMP, true);
            matched.push_back(pMP);
            if (pMP->isBad()) n_bad++;
        }
        std::map<KeyFrame*, int> counter;
        int mx = 0; KeyFrame* kmax = nullptr;
        ref_local_votes(matched, counter, kmax, mx);
        const HipKeyFrameGraph::Votes v = g.localKeyFrameVotes(F);
        CHECK(v.counter == counter && v.max_kf == kmax && v.max_count == mx && (int)v.bad_matches.size() == n_bad && n_bad > 0);
        CHECK(counter.count(A.kfs[n_kf - 1].get()) == 1);                 // the bad key frame is counted
    }

    // the culler: verdicts on the first snapshot, then the sequence in both worlds
    Params prm;
    std::vector<int> snap;
    ref_cull(A, A.kfs[0].get(), prm, &snap);
    std::vector<KeyFrame*> cands;
    for (KeyFrame* p : A.covisible) if (p->mnId != 0) cands.push_back(p);
    const std::vector<uint8_t> verdict = g.redundancy(cands, false, prm.LMobservations_thresh, prm.frac_redundant);
    std::vector<int> snap_gpu;
    for (size_t i = 0; i < cands.size(); i++) if (verdict[i]) snap_gpu.push_back(index_of(A, cands[i]));
    CHECK(snap == snap_gpu);
    const std::vector<KeyFrame*> want = ref_cull(A, A.kfs[0].get(), prm, nullptr);
    const std::vector<KeyFrame*> got = g.cullRedundant(B.kfs[0].get(), &B, prm);
    std::vector<int> wi, gi;
    for (KeyFrame* p : want) wi.push_back(index_of(A, p));
    for (KeyFrame* p : got) gi.push_back(index_of(B, p));
    CHECK(wi == gi);
    CHECK(snap == (std::vector<int>{1, 2, 3, 4, 6, 7, 8, 9, 10}) && wi == (std::vector<int>{1, 6, 7}));   // the culls changed later candidates' verdicts
    for (size_t i = 0; i < A.lms.size(); i++) CHECK(A.lms[i]->mbBad == B.lms[i]->mbBad && A.lms[i]->nObs == B.lms[i]->nObs);
    std::printf("culled on the first snapshot: %zu, in sequence: %zu\nKEYFRAME GRAPH ADAPTOR OK\n", snap.size(), wi.size());
    return 0;
}
