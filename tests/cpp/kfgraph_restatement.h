// A plain std::map restatement of CovisNode::UpdateConnections (src/core/CovisibilityGraph.cpp:42-124), the vote of
// TrackLocalMap::UpdateLocalKeyFrames (src/slam/tracking/TrackLocalMap.cpp:80-123) and KeyFrameCuller::run (src/slam/mapping/KeyFrameCuller.cpp:21-93)
// on the cv_compat.h stand-ins, and the small world they walk.  test_kfgraph_adaptor.cpp compares HipKeyFrameGraph.h with it; bench_kfgraph_ref.cpp
// times it on the table tools/bench_kfgraph.py generates.  Include cv_compat.h (or a header that does) first.
#pragma once
#include <algorithm>
#include <map>
#include <memory>
#include <set>
#include <utility>
#include <vector>

using namespace HYSLAM;

struct Params { int LMobservations_thresh = 3; float frac_redundant = 0.9f; };

struct World {
    std::vector<std::unique_ptr<KeyFrame>> kfs;
    std::vector<std::unique_ptr<MapPoint>> lms;
    std::vector<KeyFrame*> covisible;
    // the part of Map::SetBadKeyFrame the culler's later candidates can see: the key frame's observations go, a landmark left with fewer than two turns bad
    void SetBadKeyFrame(KeyFrame* pKF) {
        pKF->mbBad = true;
        for (auto& lm : lms) {
            if (lm->mObservations.erase(pKF)) { lm->nObs--; if (lm->mObservations.size() < 2) lm->mbBad = true; }
        }
    }
    std::vector<KeyFrame*> getVectorCovisibleKeyFrames(KeyFrame*) { return covisible; }
};

inline int index_of(const World& W, KeyFrame* p) { for (size_t i = 0; i < W.kfs.size(); i++) if (W.kfs[i].get() == p) return (int)i; return -1; }

inline void ref_update_connections(World& W, KeyFrame* node, int th, std::map<KeyFrame*, int>& counter, std::vector<KeyFrame*>& ordered, std::vector<int>& ws)
{
    for (MapPoint* pMP : node->GetMapPoints()) {
        if (pMP->isBad()) continue;
        for (const auto& ob : pMP->GetObservations()) {
            if (ob.first->mnId == node->mnId) continue;
            if (ob.first->isBad()) continue;
            counter[ob.first]++;
        }
    }
    if (counter.empty()) return;
    int nmax = 0; KeyFrame* kmax = nullptr;
    std::vector<std::pair<int, KeyFrame*>> pairs;
    for (const auto& kc : counter) {
        if (kc.second > nmax) { nmax = kc.second; kmax = kc.first; }
        if (kc.second >= th) pairs.push_back({kc.second, kc.first});
    }
    if (pairs.empty()) pairs.push_back({nmax, kmax});
    std::sort(pairs.begin(), pairs.end());
    for (const auto& pr : pairs) { ordered.insert(ordered.begin(), pr.second); ws.insert(ws.begin(), pr.first); }
    (void)W;
}

inline std::vector<KeyFrame*> ref_cull(World& W, KeyFrame* pKF, const Params& prm, std::vector<int>* first_snapshot,
                                       std::vector<std::pair<int, int>>* counts = nullptr)
{
    const bool is_mono = pKF->getCamera().sensor == 0;
    std::vector<KeyFrame*> culled;
    for (KeyFrame* pKFi : W.getVectorCovisibleKeyFrames(pKF)) {
        if (pKFi->mnId == 0) continue;
        const std::vector<MapPoint*> vp = pKFi->GetMapPointMatches();
        const FeatureViews& views = pKFi->getViews();
        const int thObs = prm.LMobservations_thresh;
        int nRed = 0, nMPs = 0;
        for (size_t i = 0; i < vp.size(); i++) {
            MapPoint* pMP = vp[i];
            if (!pMP || pMP->isBad()) continue;
            if (!is_mono) { const float d = views.depth((int)i); if (d > pKFi->mThDepth || d < 0) continue; }
            nMPs++;
            if (pMP->Observations() > thObs) {
                const int level = views.keypt((int)i).octave;
                int nObs = 0;
                for (const auto& ob : pMP->GetObservations()) {
                    if (ob.first == pKFi) continue;
                    if (ob.first->getViews().keypt((int)ob.second).octave <= level + 1) { nObs++; if (nObs >= thObs) break; }
                }
                if (nObs >= thObs) nRed++;
            }
        }
        const bool cull = nRed > prm.frac_redundant * nMPs;
        if (counts) counts->push_back({nMPs, nRed});
        if (first_snapshot) { if (cull) first_snapshot->push_back(index_of(W, pKFi)); }
        else if (cull) { W.SetBadKeyFrame(pKFi); culled.push_back(pKFi); }
    }
    return culled;
}

// the vote of UpdateLocalKeyFrames over a frame's matched landmarks: every observer counted, the maximum among the key frames that are not bad
inline void ref_local_votes(const std::vector<MapPoint*>& matched, std::map<KeyFrame*, int>& counter, KeyFrame*& kmax, int& mx)
{
    for (MapPoint* pMP : matched) {
        if (pMP->isBad()) continue;
        for (const auto& ob : pMP->GetObservations()) counter[ob.first]++;
    }
    mx = 0; kmax = nullptr;
    for (const auto& kc : counter) { if (kc.first->isBad()) continue; if (kc.second > mx) { mx = kc.second; kmax = kc.first; } }
}
