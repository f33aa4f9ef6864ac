// HipLandmarkEntries.h — MapPointDBEntry::_updateEntry_ (src/core/MapPointDB.cpp:223-310) for many landmarks in one call over the C ABI
// (hs_landmark_update_entries, include/hyslam_amd.h): normal and depth range, representative descriptor, mean distance and size.
//
//   HYSLAM::HipLandmarkEntries     per-landmark inputs gathered by the caller -> one HipLandmarkEntries::Result per landmark
//
// The reference runs the four steps one landmark at a time after every local / global / imaging BA (LocalBundleAdjustment.cc:197,
// GlobalBundleAdjustment.cc:173, ImagingBundleAdjustment.cc:361,424, Map.cc:351).  The hySLAM-side patch gathers each
// landmark's position, its reference key frame's camera centre, its observations (in the order of its std::map<KeyFrame*, size_t>) and its
// descriptor set (isBad() key frames left out, MapPointDB.cpp:131-135), makes ONE call and applies each Result with the entry's setters.
// The results are bit-identical to the reference's arithmetic as DESIGN.md D8 states it (a NaN only as NaN).
#pragma once
#ifdef HYSLAM_AMD_WITH_HYSLAM
#include <FeatureDescriptor.h>
#else
#include "cv_compat.h"
#endif
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/hyslam_amd.h"
#include "HipORBExtractor.h"

namespace HYSLAM {

class HipLandmarkEntries {
public:
    struct Input {
        hs_lm_entry_in entry;                          // GetWorldPos(), pKF_ref->GetCameraCenter()
        std::vector<hs_lm_obs> observations;           // one per (KeyFrame*, idx) of `observations`, in map order
        std::vector<FeatureDescriptor> descriptors;    // `descriptors` without the isBad() key frames
    };
    struct Result {
        bool normal_depth_set = false;                 // N > 0: _setNormal_, _setMaxDist_, _setMinDist_ (MapPointDB.cpp:262-264)
        cv::Mat normal;                                // 3 x 1 CV_32F when set
        float min_dist = 0.f, max_dist = 0.f;
        int best = -1, median = -1;                    // index into descriptors of _setBestDescriptor_'s argument; -1: left unchanged
        bool mean_set = false;                         // N > 0: _setMeanDistance_ (:288)
        float mean_dist = 0.f;
        float size = 0.f;                              // _setSize_ (:309), always (NaN without a positive feature size)
    };

    // `handle`: any hs_orb on the device to run on (it lends its stream and scratch); NULL = the calling thread's handle on
    // hip_detail::default_device(), created on first use.  A handle is thread-compatible: one thread at a time.
    explicit HipLandmarkEntries(hs_orb* handle = nullptr) : h(handle) { params.max_dist_factor = 2.0f; params.min_dist_factor = 0.5f; }

    // MapPointDBEntry's max_dist_invariance_factor / min_dist_invariance_factor (MapPointDB.h:99-100)
    void setFactors(float max_dist_factor, float min_dist_factor) { params.max_dist_factor = max_dist_factor; params.min_dist_factor = min_dist_factor; }

    std::vector<Result> updateEntries(const std::vector<Input>& in) {
        const size_t L = in.size();
        if (L > (size_t)INT32_MAX) throw std::invalid_argument("HipLandmarkEntries: more than 2^31 - 1 landmarks in one call");
        entries.resize(L);
        obs_off.assign(L + 1, 0);
        desc_off.assign(L + 1, 0);
        for (size_t i = 0; i < L; i++) {
            entries[i] = in[i].entry;
            obs_off[i + 1] = obs_off[i] + (int64_t)in[i].observations.size();
            desc_off[i + 1] = desc_off[i] + (int64_t)in[i].descriptors.size();
        }
        obs.resize((size_t)obs_off[L]);
        desc.resize((size_t)desc_off[L] * HS_DESC_BYTES);
        size_t k = 0, j = 0;
        for (const Input& lm : in) {
            for (const hs_lm_obs& o : lm.observations) obs[k++] = o;
            for (const FeatureDescriptor& d : lm.descriptors) {
                const cv::Mat row = d.rawDescriptor();     // the only accessor FeatureDescriptor offers (a clone)
                if (row.empty() || row.rows != 1 || row.cols != HS_DESC_BYTES || row.type() != CV_8UC1)
                    throw std::invalid_argument("HipLandmarkEntries: descriptors must be 1 x 32 CV_8UC1 (ORB)");
                std::memcpy(desc.data() + j++ * HS_DESC_BYTES, row.ptr(0), HS_DESC_BYTES);
            }
        }
        normal.resize(L * 3);
        f.resize(L * 4);
        ints.resize(L * 3);
        if (L) {
            hs_orb* use = h ? h : hip_detail::thread_handle(hip_detail::default_device().load(), "HipLandmarkEntries");
            const int st = hs_landmark_update_entries(use, &params, (int)L, entries.data(), obs_off.data(), obs.data(), desc_off.data(), desc.data(),
                                                      normal.data(), f.data(), f.data() + L, f.data() + 2 * L, f.data() + 3 * L,
                                                      ints.data(), ints.data() + L, ints.data() + 2 * L);
            if (st != HS_OK) throw std::runtime_error(std::string("HipLandmarkEntries: ") + hs_status_string(st) + ": " + hs_orb_last_error(use));
        }
        std::vector<Result> out(L);
        for (size_t i = 0; i < L; i++) {
            Result& r = out[i];
            const int flags = ints[2 * L + i];
            r.normal_depth_set = (flags & HS_LM_SET_NORMAL_DEPTH) != 0;
            if (r.normal_depth_set) {
                r.normal = cv::Mat(3, 1, CV_32F);
                for (int c = 0; c < 3; c++) r.normal.at<float>(c) = normal[3 * i + c];
                r.min_dist = f[i];
                r.max_dist = f[L + i];
            }
            r.mean_set = (flags & HS_LM_SET_MEAN) != 0;
            if (r.mean_set) r.mean_dist = f[2 * L + i];
            r.size = f[3 * L + i];
            r.best = ints[i];
            r.median = ints[L + i];
        }
        return out;
    }

private:
    hs_orb* h;
    hs_lm_entry_params params;
    std::vector<hs_lm_entry_in> entries;               // reused across calls
    std::vector<int64_t> obs_off, desc_off;
    std::vector<hs_lm_obs> obs;
    std::vector<uint8_t> desc;
    std::vector<float> normal, f;                      // f: min_dist, max_dist, mean_dist, size
    std::vector<int32_t> ints;                         // best, median, flags
};

}  // namespace HYSLAM
