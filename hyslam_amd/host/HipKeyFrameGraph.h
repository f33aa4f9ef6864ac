// HipKeyFrameGraph.h — the key-frame graph walks of hySLAM over the C ABI (hs_kf_votes, hs_kf_redundancy, hs_local_keyframes, hs_local_points,
// include/hyslam_amd.h):
//
//   updateConnections(pKF)            CovisNode::UpdateConnections (src/core/CovisibilityGraph.cpp:42-124): the counter map, the ordered key frames and
//                                     weights, and the symmetric updates the CovisGraph applies to the other nodes
//   localKeyFrameVotes(frame)         the vote of TrackLocalMap::UpdateLocalKeyFrames (src/slam/tracking/TrackLocalMap.cpp:80-123)
//   localMap(frame, map, params)      TrackLocalMap::UpdateLocalMap and the head of SearchLocalPoints (TrackLocalMap.cpp:43-67,80-184): the local key
//                                     frames, the local landmarks in the order SearchByProjection gets them, the associations to remove
//   cullRedundant(pKF, map, params)   KeyFrameCuller::run (src/slam/mapping/KeyFrameCuller.cpp:21-93) with the reference's SEQUENCE
//
// The adaptor gathers the observation table (landmark -> (key frame, octave)) from the objects, numbers the key frames by ascending address — the
// order of every std::map<KeyFrame*, ...> the reference walks — makes one call and turns slots back into pointers.  hs_kf_redundancy
// is a pure function of one snapshot of the map, and SetBadKeyFrame changes the map: cullRedundant evaluates all remaining candidates, walks them up
// to the first verdict `cull`, calls SetBadKeyFrame, regathers the snapshot and evaluates the candidates behind it again.
#pragma once
#ifdef HYSLAM_AMD_WITH_HYSLAM
#include <KeyFrame.h>
#include <Frame.h>
#include <MapPoint.h>
#else
#include "cv_compat.h"
#endif
#include <cstdint>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/hyslam_amd.h"
#include "HipORBExtractor.h"

namespace HYSLAM {

class HipKeyFrameGraph {
public:
    struct Connections {
        std::map<KeyFrame*, int> weights;              // KFcounter = mConnectedKeyFrameWeights; empty: the reference returns without touching the node
        std::vector<KeyFrame*> ordered;                // mvpOrderedConnectedKeyFrames
        std::vector<int> ordered_weights;              // mvOrderedWeights
        std::map<KeyFrame*, int> symmetric_updates;    // what UpdateConnections hands back for the other nodes (:96,103): the ordered entries
    };
    struct Votes {
        std::map<KeyFrame*, int> counter;              // keyframeCounter, the bad key frames included: local_key_frames takes an entry only if !isBad() (:113-122)
        KeyFrame* max_kf = nullptr;                    // pKFmax: the first largest count among the key frames that are not bad
        int max_count = 0;
        std::vector<int> bad_matches;                  // LMids whose landmark isBad(): the reference calls removeLandMarkAssociation on them (:96)
    };

    struct LocalMap {
        std::set<KeyFrame*> key_frames;                // local_key_frames after UpdateLocalKeyFrames; empty when nothing was counted (the reference
                                                       // then returns early and keeps the set of the frame before: the caller does the same)
        std::vector<MapPoint*> map_points;             // v_lmp handed to SearchByProjection (:74): local_map_points in ascending address
        std::vector<int> bad_matches;                  // LMids whose landmark isBad(): removeLandMarkAssociation (:62, :96)
        KeyFrame* max_kf = nullptr;                    // pKFmax
        int max_count = 0;
    };

    // `handle`: any hs_orb on the device to run on; NULL = the calling thread's handle on hip_detail::default_device().  One thread at a time.
    explicit HipKeyFrameGraph(hs_orb* handle = nullptr) : h(handle) {}

    Connections updateConnections(KeyFrame* pKF, int th = 15) {
        const std::set<MapPoint*> spMP = pKF->GetMapPoints();
        gather(std::vector<MapPoint*>(spMP.begin(), spMP.end()), false, nullptr);
        Connections out;
        const int n_kf = (int)kfs.size();
        if (n_kf == 0) return out;
        const int64_t self = (int64_t)pKF->mnId;
        vote(self, 0, th, n_kf);
        for (int s = 0; s < n_kf; s++) if (weights[s] > 0) out.weights[kfs[s]] = weights[s];
        for (int i = 0; i < n_ordered; i++) {
            out.ordered.push_back(kfs[ord_slot[i]]);
            out.ordered_weights.push_back(ord_w[i]);
            out.symmetric_updates[kfs[ord_slot[i]]] = ord_w[i];
        }
        return out;
    }

    Votes localKeyFrameVotes(Frame& frame) {
        Votes out;
        std::vector<MapPoint*> lms;
        const LandMarkMatches& matches = frame.getLandMarkMatches();
        for (auto it = matches.cbegin(); it != matches.cend(); ++it) {
            if (!it->second) continue;
            if (it->second->isBad()) out.bad_matches.push_back(it->first);
            else lms.push_back(it->second);
        }
        gather(lms, false, nullptr);
        const int n_kf = (int)kfs.size();
        if (n_kf == 0) return out;
        vote(-1, 1, 1, 0);
        for (int s = 0; s < n_kf; s++) if (weights[s] > 0) out.counter[kfs[s]] = weights[s];
        if (max_slot >= 0) { out.max_kf = kfs[max_slot]; out.max_count = max_count; }
        return out;
    }

    // `map`: HYSLAM::Map (GetAllKeyFrames, GetAllMapPoints, getBestCovisibilityKeyFrames); `params`: TrackLocalMapParameters (N_max_local_keyframes,
    // N_neighbor_keyframes).  The table is the whole map: key frames and landmarks numbered by ascending address, KeyFrame::
    // GetMapPointMatches read through the landmarks' observations (D12).  Three host-form calls; a caller that keeps the table resident chains the
    // `_device` forms instead (hs_local_map_search_device).
    template <class MapT, class Params> LocalMap localMap(Frame& frame, MapT* map, const Params& params) {
        LocalMap out;
        const int n_neighbor = params.N_neighbor_keyframes > 0 ? (int)params.N_neighbor_keyframes : 0;
        std::set<MapPoint*> lm_set;
        for (MapPoint* pMP : map->GetAllMapPoints()) if (pMP) lm_set.insert(pMP);
        std::vector<int> lmids;
        std::vector<MapPoint*> held;
        const LandMarkMatches& matches = frame.getLandMarkMatches();
        for (auto it = matches.cbegin(); it != matches.cend(); ++it) { lmids.push_back(it->first); held.push_back(it->second); if (it->second) lm_set.insert(it->second); }
        const std::vector<MapPoint*> lms(lm_set.begin(), lm_set.end());
        // every key frame the walk can reach: the map's, the observers, and their neighbours and parents
        std::set<KeyFrame*> reach;
        for (KeyFrame* pKF : map->GetAllKeyFrames()) if (pKF) reach.insert(pKF);
        for (MapPoint* pMP : lms) if (!pMP->isBad()) for (const auto& kv : pMP->GetObservations()) reach.insert(kv.first);
        std::vector<KeyFrame*> todo(reach.begin(), reach.end());
        std::map<KeyFrame*, std::vector<KeyFrame*>> best;
        while (!todo.empty()) {
            KeyFrame* pKF = todo.back(); todo.pop_back();
            std::vector<KeyFrame*>& row = best[pKF];
            row = map->getBestCovisibilityKeyFrames(pKF, n_neighbor);
            if ((int)row.size() > n_neighbor) row.resize((size_t)n_neighbor);
            for (KeyFrame* q : row) if (q && reach.insert(q).second) todo.push_back(q);
            KeyFrame* par = pKF->GetParent();
            if (par && reach.insert(par).second) todo.push_back(par);
        }
        const std::vector<KeyFrame*> also(reach.begin(), reach.end());
        gather(lms, false, &also);
        const int n_kf = (int)kfs.size();
        std::unordered_map<MapPoint*, int32_t> index;
        for (size_t i = 0; i < lms.size(); i++) index[lms[i]] = (int32_t)i;
        std::vector<int32_t> frame_lm(held.size(), -1);
        for (size_t i = 0; i < held.size(); i++) if (held[i]) frame_lm[i] = index.at(held[i]);
        if (n_kf > 0) {
            vote(-1, 1, 1, 0, &frame_lm);
            if (max_slot >= 0) { out.max_kf = kfs[max_slot]; out.max_count = max_count; }
        } else weights.clear();
        std::vector<int32_t> neigh((size_t)n_kf * n_neighbor, -1), parent((size_t)n_kf, -1);
        for (int s = 0; s < n_kf; s++) {
            const std::vector<KeyFrame*>& row = best[kfs[s]];
            for (size_t k = 0; k < row.size(); k++) if (row[k]) neigh[(size_t)s * n_neighbor + k] = slot_of.at(row[k]);
            if (KeyFrame* par = kfs[s]->GetParent()) parent[s] = slot_of.at(par);
        }
        std::vector<uint8_t> local((size_t)n_kf, 0), remove(frame_lm.size(), 0);
        std::vector<int32_t> sel(lms.size(), -1);
        int32_t n_local = 0, n_sel = 0;
        const hs_kf_table T = table();
        hs_orb* use = handle();
        int st = hs_local_keyframes(use, n_kf, weights.data(), kf_bad.data(), neigh.data(), n_neighbor, parent.data(), (int)params.N_max_local_keyframes,
                                    n_neighbor, local.data(), &n_local);
        if (st != HS_OK) fail(use, st);
        st = hs_local_points(use, &T, local.data(), frame_lm.data(), (int)frame_lm.size(), remove.data(), sel.data(), (int)sel.size(), &n_sel);
        if (st != HS_OK) fail(use, st);
        for (int s = 0; s < n_kf; s++) if (local[s]) out.key_frames.insert(kfs[s]);
        for (int32_t j = 0; j < n_sel; j++) out.map_points.push_back(lms[sel[j]]);
        for (size_t i = 0; i < remove.size(); i++) if (remove[i]) out.bad_matches.push_back(lmids[i]);
        return out;
    }

    // `map`: HYSLAM::Map (getVectorCovisibleKeyFrames, SetBadKeyFrame); `params`: KeyFrameCullerParameters (LMobservations_thresh, frac_redundant).
    // Returns the key frames SetBadKeyFrame was called on, in the reference's order.
    template <class MapT, class Params> std::vector<KeyFrame*> cullRedundant(KeyFrame* pKF, MapT* map, const Params& params) {
        const bool is_mono = pKF->getCamera().sensor == 0;
        std::vector<KeyFrame*> cands;
        for (KeyFrame* pKFi : map->getVectorCovisibleKeyFrames(pKF)) if (pKFi->mnId != 0) cands.push_back(pKFi);      // (:31)
        std::vector<KeyFrame*> culled;
        size_t pos = 0;
        while (pos < cands.size()) {
            const std::vector<uint8_t> cull = redundancy(std::vector<KeyFrame*>(cands.begin() + pos, cands.end()), is_mono,
                                                         params.LMobservations_thresh, params.frac_redundant);
            size_t i = 0;
            while (i < cull.size() && !cull[i]) i++;
            if (i == cull.size()) break;
            map->SetBadKeyFrame(cands[pos + i]);                      // changes the snapshot: everything behind it is evaluated again
            culled.push_back(cands[pos + i]);
            pos += i + 1;
        }
        return culled;
    }

    // the verdict of every candidate against the map as it is now (n_mps / n_redundant of the last call stay readable)
    std::vector<uint8_t> redundancy(const std::vector<KeyFrame*>& cands, bool is_mono, int th_obs, float frac_redundant) {
        std::vector<MapPoint*> lms;
        std::unordered_map<MapPoint*, int32_t> index;
        std::vector<int64_t> c_off(1, 0);
        std::vector<int32_t> item_lm, item_oct, c_slot;
        std::vector<float> item_depth, c_th;
        for (KeyFrame* pKFi : cands) {
            const std::vector<MapPoint*> vp = pKFi->GetMapPointMatches();
            const FeatureViews& views = pKFi->getViews();
            for (size_t i = 0; i < vp.size(); i++) {
                if (!vp[i]) continue;
                const auto ins = index.insert({vp[i], (int32_t)lms.size()});
                if (ins.second) lms.push_back(vp[i]);
                item_lm.push_back(ins.first->second);
                item_oct.push_back(views.keypt((int)i).octave);
                item_depth.push_back(views.depth((int)i));
            }
            c_off.push_back((int64_t)item_lm.size());
            c_th.push_back(pKFi->mThDepth);
        }
        gather(lms, true, &cands);
        for (KeyFrame* pKFi : cands) c_slot.push_back(slot_of.at(pKFi));
        const size_t C = cands.size();
        n_mps.assign(C, 0); n_redundant.assign(C, 0);
        std::vector<uint8_t> cull(C, 0);
        if (C == 0) return cull;
        const hs_kf_table T = table();
        hs_orb* use = handle();
        const int st = hs_kf_redundancy(use, &T, (int)C, c_slot.data(), c_th.data(), c_off.data(), item_lm.data(), item_oct.data(), item_depth.data(),
                                        is_mono ? 1 : 0, th_obs, frac_redundant, n_mps.data(), n_redundant.data(), cull.data());
        if (st != HS_OK) fail(use, st);
        return cull;
    }
    std::vector<int32_t> n_mps, n_redundant;

private:
    hs_orb* handle() { return h ? h : hip_detail::thread_handle(hip_detail::default_device().load(), "HipKeyFrameGraph"); }
    [[noreturn]] static void fail(hs_orb* use, int st) { throw std::runtime_error(std::string("HipKeyFrameGraph: ") + hs_status_string(st) + ": " + hs_orb_last_error(use)); }

    // the observation table of `lms` (landmark i = lms[i]); key frames = every observer (+ `also`), numbered by ascending address
    void gather(const std::vector<MapPoint*>& lms, bool with_octaves, const std::vector<KeyFrame*>* also) {
        std::vector<std::map<KeyFrame*, size_t>> obs(lms.size());
        std::set<KeyFrame*> all;
        if (also) all.insert(also->begin(), also->end());
        lm_bad.assign(lms.size(), 0); lm_nobs.assign(lms.size(), 0);
        for (size_t i = 0; i < lms.size(); i++) {
            lm_bad[i] = lms[i]->isBad() ? 1 : 0;
            if (lm_bad[i]) continue;                                  // contributes nothing: its observations are not gathered
            lm_nobs[i] = lms[i]->Observations();
            obs[i] = lms[i]->GetObservations();
            for (const auto& kv : obs[i]) all.insert(kv.first);
        }
        kfs.assign(all.begin(), all.end());
        slot_of.clear();
        kf_bad.resize(kfs.size()); kf_id.resize(kfs.size());
        for (size_t s = 0; s < kfs.size(); s++) { slot_of[kfs[s]] = (int32_t)s; kf_bad[s] = kfs[s]->isBad() ? 1 : 0; kf_id[s] = (int64_t)kfs[s]->mnId; }
        lm_off.assign(1, 0); lm_kf.clear(); lm_oct.clear();
        for (size_t i = 0; i < lms.size(); i++) {
            for (const auto& kv : obs[i]) {                           // a std::map<KeyFrame*, size_t>: ascending address = ascending slot
                lm_kf.push_back(slot_of[kv.first]);
                lm_oct.push_back(with_octaves ? kv.first->getViews().keypt((int)kv.second).octave : 0);
            }
            lm_off.push_back((int64_t)lm_kf.size());
        }
        n_lms = (int32_t)lms.size();
    }
    hs_kf_table table() const {
        hs_kf_table T;
        T.L = n_lms; T.n_kf = (int32_t)kfs.size();
        T.lm_obs_offsets = lm_off.data(); T.lm_obs_kf = lm_kf.data(); T.lm_obs_octave = lm_oct.data();
        T.lm_bad = lm_bad.data(); T.lm_nobs = lm_nobs.data(); T.kf_bad = kf_bad.data(); T.kf_id = kf_id.data();
        return T;
    }
    // one query: over all gathered landmarks, or over those `only` lists (-1 entries left out)
    void vote(int64_t self, int count_bad_kf, int th, int cap, const std::vector<int32_t>* only = nullptr) {
        const int n_kf = (int)kfs.size();
        std::vector<int32_t> q_lm;
        if (only) { for (int32_t i : *only) if (i >= 0) q_lm.push_back(i); }
        else { q_lm.resize((size_t)n_lms); for (int32_t i = 0; i < n_lms; i++) q_lm[i] = i; }
        const int64_t q_off[2] = {0, (int64_t)q_lm.size()};
        weights.assign((size_t)n_kf, 0); ord_slot.assign((size_t)cap + 1, -1); ord_w.assign((size_t)cap + 1, 0);
        const hs_kf_table T = table();
        hs_orb* use = handle();
        const int st = hs_kf_votes(use, &T, 1, q_off, q_lm.data(), &self, count_bad_kf, th, weights.data(), &max_slot, &max_count,
                                   ord_slot.data(), ord_w.data(), cap, &n_ordered);
        if (st != HS_OK) fail(use, st);
        if (n_ordered > cap) n_ordered = cap;
    }

    hs_orb* h;
    std::vector<KeyFrame*> kfs;                        // slot -> key frame
    std::map<KeyFrame*, int32_t> slot_of;
    std::vector<int64_t> lm_off, kf_id;
    std::vector<int32_t> lm_kf, lm_oct, lm_nobs, weights, ord_slot, ord_w;
    std::vector<uint8_t> lm_bad, kf_bad;
    int32_t n_lms = 0, max_slot = -1, max_count = 0, n_ordered = 0;
};

}  // namespace HYSLAM
