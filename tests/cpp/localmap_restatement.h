// A literal restatement of TrackLocalMap::UpdateLocalKeyFrames, UpdateLocalPoints and the head of SearchLocalPoints
// (src/slam/tracking/TrackLocalMap.cpp:55-67,80-184) on the cv_compat.h stand-ins: the std::set<KeyFrame*> iterated while it grows, each local key
// frame's GetMapPointMatches(), the erase of what the frame already holds — and the map it walks.  test_localmap_adaptor.cpp compares
// HipKeyFrameGraph::localMap with it; bench_localmap_ref.cpp times it on the table tools/bench_local_map.py generates.  Include cv_compat.h (or a
// header that does) first.
#pragma once
#include "kfgraph_restatement.h"

struct TrackLocalMapParameters { int N_max_local_keyframes = 80; int N_neighbor_keyframes = 10; };

struct MapWorld : World {
    std::map<KeyFrame*, std::vector<KeyFrame*>> ordered;               // mvpOrderedConnectedKeyFrames of every node
    std::vector<KeyFrame*> GetAllKeyFrames() { std::vector<KeyFrame*> v; for (auto& k : kfs) v.push_back(k.get()); return v; }
    std::vector<MapPoint*> GetAllMapPoints() { std::vector<MapPoint*> v; for (auto& l : lms) v.push_back(l.get()); return v; }
    std::vector<KeyFrame*> getBestCovisibilityKeyFrames(KeyFrame* pKF, const int& N) {      // CovisNode::GetBestCovisibilityKeyFrames: the first N
        const std::vector<KeyFrame*>& o = ordered[pKF];
        return (int)o.size() <= N ? o : std::vector<KeyFrame*>(o.begin(), o.begin() + N);
    }
};

// TrackLocalMap.cpp:80-184 and :55-67, statement by statement
struct Literal { std::set<KeyFrame*> local_key_frames; std::vector<MapPoint*> v_lmp; std::vector<int> removed; };
inline Literal literal(Frame& F, MapWorld* pMap, const TrackLocalMapParameters& params)
{
    Literal out;
    std::set<KeyFrame*>& local_key_frames = out.local_key_frames;
    std::set<MapPoint*> local_map_points;
    std::map<KeyFrame*, int> keyframeCounter;
    const LandMarkMatches matches = F.getLandMarkMatches();
    for (auto it = matches.cbegin(); it != matches.cend(); ++it) {
        MapPoint* pMP = it->second;
        if (!pMP) continue;
        if (!pMP->isBad()) { for (const auto& ob : pMP->GetObservations()) keyframeCounter[ob.first]++; }
        else out.removed.push_back(it->first);
    }
    if (!keyframeCounter.empty()) {
        for (const auto& kc : keyframeCounter) { if (kc.first->isBad()) continue; local_key_frames.insert(kc.first); }
        for (auto itKF = local_key_frames.begin(), itEndKF = local_key_frames.end(); itKF != itEndKF; itKF++) {
            if (local_key_frames.size() > (size_t)params.N_max_local_keyframes) break;
            KeyFrame* pKF = *itKF;
            const std::vector<KeyFrame*> vNeighs = pMap->getBestCovisibilityKeyFrames(pKF, params.N_neighbor_keyframes);
            for (KeyFrame* pNeighKF : vNeighs) { if (!pNeighKF->isBad()) { local_key_frames.insert(pNeighKF); break; } }
            KeyFrame* pParent = pKF->GetParent();
            if (pParent) { local_key_frames.insert(pParent); break; }
        }
    }
    for (KeyFrame* pKF : local_key_frames) {
        for (MapPoint* pMP : pKF->GetMapPointMatches()) { if (!pMP) continue; if (!pMP->isBad()) local_map_points.insert(pMP); }
    }
    for (auto it = matches.cbegin(); it != matches.cend(); ++it) {
        MapPoint* pMP = it->second;
        if (!pMP) continue;
        if (!pMP->isBad()) local_map_points.erase(pMP);
    }
    out.v_lmp.assign(local_map_points.begin(), local_map_points.end());
    return out;
}
