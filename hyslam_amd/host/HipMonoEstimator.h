// HipMonoEstimator.h — MonoEstimator (src/initializers/MonoEstimator.h:48-60) over the C ABI (hs_monoinit_estimate, include/hyslam_amd.h): the
// reference's public surface,
//
//   HipMonoEstimator(ReferenceFrame, params)                                      keeps the reference frame's key points and camera (:32-44)
//   Initialize(CurrentFrame, vMatches12, R21, t21, vP3D, vbTriangulated)          the reference's signature and return value
//
// and one call for all monocular cameras of a rig:
//
//   HipMonoEstimator::Initialize(estimators, frames, matches, results)            static: ONE hs_monoinit_estimate for every estimator of the list
//
// The call keeps no state.  `seed` replaces SeedRandOnce(0) + RandomInt.  Where Initialize returns false the reference leaves R21,
// t21, vP3D and vbTriangulated as they were; so does the member form.  The parallax is reported as a cosine: parallax_deg converts.
#pragma once
#ifdef HYSLAM_AMD_WITH_HYSLAM
#include <Frame.h>
#include <MonoEstimator.h>
#else
#include "cv_compat.h"
#endif
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/hyslam_amd.h"
#include "HipORBExtractor.h"
#include "HipRansacBatch.h"

namespace HYSLAM {

class HipMonoEstimator {
public:
    // what one estimator's part of a call gave: Initialize's return value and outputs, and the record
    struct Result {
        bool ok = false; cv::Mat R21, t21; std::vector<cv::Point3f> vP3D; std::vector<bool> vbTriangulated;
        std::vector<uint8_t> inliers_h, inliers_f;                 // by COMPACTED match, n1 long
        hs_monoinit_result info;
    };

    HipMonoEstimator(const Frame& ReferenceFrame, MonoEstimatorParams params, uint64_t seed = 0, hs_orb* handle = nullptr) : handle_(handle)
    {
        gather(ReferenceFrame.getViews().getKeys(), keys1_);
        const Camera& c = ReferenceFrame.getCamera();
        params_ = hs_monoinit_params();
        params_.fx = c.fx(); params_.fy = c.fy(); params_.cx = c.cx(); params_.cy = c.cy();
        params_.sigma = params.sigma; params_.max_iterations = params.MaxIterations; params_.min_triangulated = params.minTriangulated;
        params_.min_frac_triangulated = params.minFracTriangulated;
        params_.min_parallax_deg = 1.0f;                           // the 1.0 Initialize hands to ReconstructH / ReconstructF (:130-132)
        params_.seed = seed;
    }

    bool Initialize(const Frame& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21, std::vector<cv::Point3f>& vP3D,
                    std::vector<bool>& vbTriangulated)
    {
        std::vector<HipMonoEstimator*> one(1, this);
        std::vector<const Frame*> frames(1, &CurrentFrame);
        std::vector<const std::vector<int>*> matches(1, &vMatches12);
        std::vector<Result> r;
        Initialize(one, frames, matches, r);
        if (!r[0].ok) return false;
        R21 = r[0].R21; t21 = r[0].t21; vP3D = r[0].vP3D; vbTriangulated = r[0].vbTriangulated;
        return true;
    }

    // Initialize of every estimator in one call; results[q] belongs to estimators[q].  All run on the first one's handle.  vMatches12 of estimator q
    // holds one entry per key point of its reference frame.
    static void Initialize(const std::vector<HipMonoEstimator*>& estimators, const std::vector<const Frame*>& frames,
                           const std::vector<const std::vector<int>*>& matches, std::vector<Result>& results)
    {
        const int Q = (int)estimators.size();
        results.assign(Q, Result());
        if (Q == 0) return;
        if ((int)frames.size() != Q || (int)matches.size() != Q) throw std::invalid_argument("HipMonoEstimator: one frame and one match vector per estimator");
        std::vector<hs_monoinit_params> par(Q);
        std::vector<int64_t> off1(Q + 1, 0), off2(Q + 1, 0);
        std::vector<hs_keypoint> k1, k2;
        std::vector<int32_t> m12;
        for (int q = 0; q < Q; q++) {
            const HipMonoEstimator& e = *estimators[q];
            if (matches[q]->size() != e.keys1_.size()) throw std::invalid_argument("HipMonoEstimator: vMatches12 holds one entry per key point of the reference frame");
            par[q] = e.params_;
            k1.insert(k1.end(), e.keys1_.begin(), e.keys1_.end());
            gather(frames[q]->getViews().getKeys(), k2);
            m12.insert(m12.end(), matches[q]->begin(), matches[q]->end());
            off1[q + 1] = (int64_t)k1.size(); off2[q + 1] = (int64_t)k2.size();
        }
        const size_t n1 = k1.size();
        std::vector<hs_monoinit_result> res(Q);
        std::vector<uint8_t> ih(n1 + 1), jf(n1 + 1), tri(n1 + 1);
        std::vector<float> p3d(3 * n1 + 1);
        if (k1.empty()) k1.resize(1);
        if (k2.empty()) k2.resize(1);
        if (m12.empty()) m12.resize(1);
        hs_orb* use = hip_detail::batch_handle(estimators[0]->handle_, "HipMonoEstimator");
        hip_detail::batch_check(hs_monoinit_estimate(use, Q, par.data(), off1.data(), k1.data(), off2.data(), k2.data(), m12.data(), nullptr, 0, res.data(), ih.data(), jf.data(),
                                                     p3d.data(), tri.data()), use, "HipMonoEstimator");
        for (int q = 0; q < Q; q++) {
            Result& r = results[q];
            r.info = res[q];
            r.ok = res[q].status == HS_MONOINIT_OK_H || res[q].status == HS_MONOINIT_OK_F;       // a pose with a NaN (HS_MONOINIT_NONFINITE) is a failure
            r.inliers_h.assign(ih.begin() + off1[q], ih.begin() + off1[q + 1]);
            r.inliers_f.assign(jf.begin() + off1[q], jf.begin() + off1[q + 1]);
            const size_t n = (size_t)(off1[q + 1] - off1[q]);
            r.vP3D.assign(n, cv::Point3f()); r.vbTriangulated.assign(n, false);
            for (size_t i = 0; i < n; i++) {
                const size_t g = (size_t)off1[q] + i;
                r.vP3D[i] = cv::Point3f(p3d[3 * g], p3d[3 * g + 1], p3d[3 * g + 2]);
                r.vbTriangulated[i] = tri[g] != 0;
            }
            if (!r.ok) continue;                                   // no pose: empty cv::Mat
            r.R21 = cv::Mat(3, 3, CV_32F); r.t21 = cv::Mat(3, 1, CV_32F);
            for (int i = 0; i < 9; i++) r.R21.at<float>(i / 3, i % 3) = res[q].R21[i];
            for (int i = 0; i < 3; i++) r.t21.at<float>(i) = res[q].t21[i];
        }
    }

    // the reference's parallax of the motion that decided, in degrees, from the cosine the library reports
    static double parallax_deg(const hs_monoinit_result& info) {
        const double c = info.cos_parallax > 1.0f ? 1.0 : info.cos_parallax < -1.0f ? -1.0 : (double)info.cos_parallax;
        return std::acos(c) * 180.0 / 3.14159265358979323846;
    }

    const std::vector<hs_keypoint>& keys() const { return keys1_; }
    const hs_monoinit_params& params() const { return params_; }

private:
    static void gather(const std::vector<cv::KeyPoint>& keys, std::vector<hs_keypoint>& out) {
        for (const cv::KeyPoint& k : keys) {
            hs_keypoint o = hs_keypoint();
            o.x = k.pt.x; o.y = k.pt.y; o.size = k.size; o.angle = k.angle; o.response = k.response; o.octave = k.octave;
            out.push_back(o);
        }
    }
    hs_orb* handle_;
    std::vector<hs_keypoint> keys1_;
    hs_monoinit_params params_;
};

}  // namespace HYSLAM
