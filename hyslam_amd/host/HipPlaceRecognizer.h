// HipPlaceRecognizer.h — HYSLAM::PlaceRecognizer (src/core/PlaceRecognizer.cpp:43-311) for ONE database level of KeyFrameDB over the C ABI
// (hs_place_db_*, hs_place_query_*, include/hyslam_amd.h): the key frames' BoW vectors live in HBM, a query is one score pass over all of them.
//
//   HYSLAM::HipPlaceRecognizer     add / erase / clear / detectRelocalizationCandidates / detectLoopCandidates
//
// The core works on plain data: a key frame is a uint64_t key (the KeyFrame* value: it orders the results wherever the reference orders by address,
// DESIGN.md D6), its BoW vector any std::map<word, value> (DBoW2::BowVector), its covisibility a list of keys.  Under HYSLAM_AMD_WITH_HYSLAM the
// KeyFrame* overloads gather mBowVec on add and GetBestCovisibilityKeyFrames(10) / GetConnectedKeyFrames() at query time, and return what
// KeyFrameDB::DetectRelocalizationCandidates / DetectLoopCandidates hand on (KeyFrameDB.cc:392-419); the sub_dbs recursion stays in hySLAM
// (INTEGRATION.md §10).  One deviation from the reference is documented as DESIGN.md D9.
//
// Threading: as the class it replaces (mMutex, PlaceRecognizer.cpp:45,55,90,207), every member function takes the object's own mutex: KeyFrameDB
// adds and erases from LocalMapping while LoopClosing and Tracking query.  The object OWNS its hs_orb handle (made in the constructor on the given
// device), so no other adaptor or thread shares the stream, the scratch or the lifetime of the handle the database runs on.
#pragma once
#ifdef HYSLAM_AMD_WITH_HYSLAM
#include <KeyFrame.h>
#include <Frame.h>
#endif
#include <cstdint>
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/hyslam_amd.h"
#include "HipORBExtractor.h"

namespace HYSLAM {

class HipPlaceRecognizer {
public:
    using Key = uint64_t;
    using Neighbours = std::function<std::vector<Key>(Key)>;     // GetBestCovisibilityKeyFrames(10) of a key frame, in that call's order

    // n_words: FeatureVocabulary::size() (setVocab, :36-40).  device < 0: hip_detail::default_device().  The object creates and owns a handle of
    // its own on that device (never a thread's shared one): it is used under `mutex` only and lives exactly as long as the database.
    explicit HipPlaceRecognizer(int n_words, int device = -1) {
        hs_orb_params p;
        hs_orb_default_params(&p);
        int st = hs_orb_create(&p, device >= 0 ? device : hip_detail::default_device().load(), &h);
        if (st != HS_OK) throw std::runtime_error(std::string("HipPlaceRecognizer: ") + hs_status_string(st));
        st = hs_place_db_create(h, n_words, 0 /*L1_NORM*/, &db);
        if (st != HS_OK) { const std::string msg = std::string("HipPlaceRecognizer: ") + hs_status_string(st) + ": " + hs_orb_last_error(h); hs_orb_destroy(h); throw std::runtime_error(msg); }
    }
    ~HipPlaceRecognizer() { hs_place_db_destroy(db); hs_orb_destroy(h); }
    HipPlaceRecognizer(const HipPlaceRecognizer&) = delete;
    HipPlaceRecognizer& operator=(const HipPlaceRecognizer&) = delete;

    template <class BowMap> void add(Key key, const BowMap& bow) {
        std::lock_guard<std::mutex> lock(mutex);
        if (slot_of.count(key)) throw std::invalid_argument("HipPlaceRecognizer: key already in the database");
        flatten(bow);
        int32_t slot = -1;
        const int st = hs_place_db_add(db, key, qw.data(), qv.data(), (int)qw.size(), &slot);
        if (st != HS_OK) fail(st);
        slot_of[key] = slot;
        if ((size_t)slot >= key_of.size()) key_of.resize((size_t)slot + 1);
        key_of[slot] = key;
    }
    void erase(Key key) {
        std::lock_guard<std::mutex> lock(mutex);
        const auto it = slot_of.find(key);
        if (it == slot_of.end()) return;                         // the reference's erase of an unknown key frame finds nothing to remove
        const int st = hs_place_db_erase(db, it->second);
        if (st != HS_OK) fail(st);
        slot_of.erase(it);
    }
    void clear() {
        std::lock_guard<std::mutex> lock(mutex);
        const int st = hs_place_db_clear(db);
        if (st != HS_OK) fail(st);
        slot_of.clear(); key_of.clear();
    }
    size_t size() const { std::lock_guard<std::mutex> lock(mutex); return slot_of.size(); }

    // the candidates in ascending key order: what iterating KeyFrameDB's std::set<KeyFrame*> gives (KeyFrameDB.cc:392-405)
    template <class BowMap> std::vector<Key> detectRelocalizationCandidates(const BowMap& bow, const Neighbours& neighbours) {
        return query(false, bow, neighbours, nullptr, 0.0f);
    }
    // pBestKF of every retained entry in the reference's walk order (:184-195); `connected`: GetConnectedKeyFrames() of the query key frame
    template <class BowMap> std::vector<Key> detectLoopCandidates(const BowMap& bow, const std::set<Key>& connected, float minScore, const Neighbours& neighbours) {
        return query(true, bow, neighbours, &connected, minScore);
    }

#ifdef HYSLAM_AMD_WITH_HYSLAM
    static Key keyOf(const KeyFrame* pKF) { return (Key)(uintptr_t)pKF; }
    void add(KeyFrame* pKF) { add(keyOf(pKF), pKF->mBowVec); }
    void erase(KeyFrame* pKF) { erase(keyOf(pKF)); }
    std::vector<KeyFrame*> detectLoopCandidates(KeyFrame* pKF, float minScore) {
        std::set<Key> connected;
        for (KeyFrame* c : pKF->GetConnectedKeyFrames()) connected.insert(keyOf(c));
        return pointers(detectLoopCandidates(pKF->mBowVec, connected, minScore, covisibility()));
    }
    std::vector<KeyFrame*> detectRelocalizationCandidates(Frame* F) { return pointers(detectRelocalizationCandidates(F->mBowVec, covisibility())); }
    // as KeyFrameDB::DetectRelocalizationCandidates collects them for one level
    std::set<KeyFrame*> relocalizationCandidateSet(Frame* F) {
        const std::vector<KeyFrame*> v = detectRelocalizationCandidates(F);
        return std::set<KeyFrame*>(v.begin(), v.end());
    }
#endif

private:
    [[noreturn]] void fail(int st) const { throw std::runtime_error(std::string("HipPlaceRecognizer: ") + hs_status_string(st) + ": " + hs_orb_last_error(h)); }

    template <class BowMap> void flatten(const BowMap& bow) {
        qw.clear(); qv.clear();
        for (const auto& wv : bow) { qw.push_back((int32_t)wv.first); qv.push_back((double)wv.second); }     // a std::map: ascending words
    }

    template <class BowMap> std::vector<Key> query(bool loop, const BowMap& bow, const Neighbours& neighbours, const std::set<Key>* connected, float min_score) {
        // the covisibility lists are gathered BEFORE the lock: `neighbours` calls into the caller's objects (KeyFrame::GetBestCovisibilityKeyFrames takes
        // the key frame's own mutex), and nothing of this object is touched until they are all here
        std::vector<Key> live;
        {
            std::lock_guard<std::mutex> lock(mutex);
            live.reserve(slot_of.size());
            for (const auto& ks : slot_of) live.push_back(ks.first);
        }
        std::vector<std::vector<Key>> lists(live.size());
        if (neighbours) for (size_t i = 0; i < live.size(); i++) lists[i] = neighbours(live[i]);
        std::lock_guard<std::mutex> lock(mutex);
        flatten(bow);
        const size_t slots = key_of.size();
        neigh.assign(slots * 10, -1);
        for (size_t i = 0; i < live.size(); i++) {
            const auto self = slot_of.find(live[i]);
            if (self == slot_of.end()) continue;                                                           // erased while the lists were gathered
            size_t n = 0;
            for (Key nb : lists[i]) {
                const auto it = slot_of.find(nb);
                if (it != slot_of.end() && n < 10) neigh[(size_t)self->second * 10 + n++] = it->second;       // not in this database: not in its inverted file
            }
        }
        cand.assign(slots ? slots : 1, -1);
        int32_t n_cand = 0;
        int st;
        if (loop) {
            excl.assign(slots ? slots : 1, 0);
            for (Key c : *connected) { const auto it = slot_of.find(c); if (it != slot_of.end()) excl[it->second] = 1; }
            st = hs_place_query_loop(db, qw.data(), qv.data(), (int)qw.size(), excl.data(), min_score, neigh.data(), cand.data(), (int)slots, &n_cand,
                                     nullptr, nullptr, nullptr, nullptr);
        } else {
            st = hs_place_query_reloc(db, qw.data(), qv.data(), (int)qw.size(), neigh.data(), cand.data(), (int)slots, &n_cand, nullptr, nullptr, nullptr, nullptr);
        }
        if (st != HS_OK) fail(st);
        std::vector<Key> out((size_t)n_cand);
        for (int32_t i = 0; i < n_cand; i++) out[i] = key_of[cand[i]];
        return out;
    }

#ifdef HYSLAM_AMD_WITH_HYSLAM
    static Neighbours covisibility() {
        return [](Key k) {
            std::vector<Key> out;
            for (KeyFrame* nb : reinterpret_cast<KeyFrame*>((uintptr_t)k)->GetBestCovisibilityKeyFrames(10)) out.push_back(keyOf(nb));
            return out;
        };
    }
    static std::vector<KeyFrame*> pointers(const std::vector<Key>& keys) {
        std::vector<KeyFrame*> out;
        for (Key k : keys) out.push_back(reinterpret_cast<KeyFrame*>((uintptr_t)k));
        return out;
    }
#endif

    mutable std::mutex mutex;                                    // guards everything below, as PlaceRecognizer::mMutex does
    hs_orb* h = nullptr;                                         // owned
    hs_place_db* db = nullptr;
    std::unordered_map<Key, int32_t> slot_of;                    // live entries
    std::vector<Key> key_of;                                     // slot -> key
    std::vector<int32_t> qw, neigh, cand;                        // reused across calls
    std::vector<double> qv;
    std::vector<uint8_t> excl;
};

}  // namespace HYSLAM
