// HipLandmarkDescriptors.h — MapPointDBEntry::_computeDistinctiveDescriptor_ (src/core/MapPointDB.cpp:128-175) for many landmarks in one call
// over the C ABI (hs_landmark_best_descriptors, include/hyslam_amd.h).
//
//   HYSLAM::HipLandmarkDescriptors     observations of L landmarks -> the index of each landmark's representative descriptor
//
// The reference recomputes this one landmark at a time on the mapping thread (after every local / global / imaging BA, Map::_addAssociation_,
// _eraseAssociation_).  The hySLAM-side patch collects the landmarks of such a loop, makes ONE batched call and hands the chosen
// descriptor to _setBestDescriptor_.  Each inner vector holds one landmark's observation descriptors in the order the reference iterates its
// std::map<KeyFrame*, FeatureDescriptor> — sorted by KeyFrame address, isBad() key frames left out (MapPointDB.cpp:131-135).  Only the
// descriptor choice moves to the GPU: _updateNormalAndDepth_ / _updateMeanDistance_ (cv::norm float arithmetic) stay on the host.
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

class HipLandmarkDescriptors {
public:
    // `handle`: any hs_orb on the device to run on (it lends its stream and scratch); NULL = the calling thread's handle on
    // hip_detail::default_device(), created on first use.  A handle is thread-compatible: one thread at a time.
    explicit HipLandmarkDescriptors(hs_orb* handle = nullptr) : h(handle) {}

    // best[i] = index into observations[i] of landmark i's representative descriptor (the reference's BestIdx), -1 for a landmark without
    // observations (the reference leaves such a landmark unchanged).  `medians`, when given, receives that row's median Hamming distance (-1 likewise).
    std::vector<int> bestDescriptors(const std::vector<std::vector<FeatureDescriptor>>& observations, std::vector<int>* medians = nullptr) {
        const size_t L = observations.size();
        if (L > (size_t)INT32_MAX) throw std::invalid_argument("HipLandmarkDescriptors: more than 2^31 - 1 landmarks in one call");
        offsets.assign(L + 1, 0);
        for (size_t i = 0; i < L; i++) offsets[i + 1] = offsets[i] + (int64_t)observations[i].size();
        desc.resize((size_t)offsets[L] * HS_DESC_BYTES);
        size_t k = 0;
        for (const auto& lm : observations)
            for (const auto& d : lm) {
                const cv::Mat row = d.rawDescriptor();      // the only accessor FeatureDescriptor offers (a clone)
                if (row.empty() || row.rows != 1 || row.cols != HS_DESC_BYTES || row.type() != CV_8UC1)
                    throw std::invalid_argument("HipLandmarkDescriptors: descriptors must be 1 x 32 CV_8UC1 (ORB)");
                std::memcpy(desc.data() + k++ * HS_DESC_BYTES, row.ptr(0), HS_DESC_BYTES);
            }
        std::vector<int32_t> best(L), med(L);
        if (L) {
            hs_orb* use = h ? h : hip_detail::thread_handle(hip_detail::default_device().load(), "HipLandmarkDescriptors");
            const int st = hs_landmark_best_descriptors(use, offsets.data(), desc.data(), (int)L, best.data(), med.data());
            if (st != HS_OK) throw std::runtime_error(std::string("HipLandmarkDescriptors: ") + hs_status_string(st) + ": " + hs_orb_last_error(use));
        }
        if (medians) medians->assign(med.begin(), med.end());
        return std::vector<int>(best.begin(), best.end());
    }

private:
    hs_orb* h;
    std::vector<int64_t> offsets;       // reused across calls
    std::vector<uint8_t> desc;
};

}  // namespace HYSLAM
