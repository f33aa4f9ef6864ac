// HipSim3Solver.h — Sim3Solver (src/estimators/Sim3Solver.h:36-52) over the C ABI (hs_sim3_iterate, include/hyslam_amd.h): the reference's public surface,
//
//   HipSim3Solver(pKF1, pKF2, vpMatched12, bFixScale)     gathers the correspondences in ascending i1 as the reference's constructor does (:66-107)
//   SetRansacParameters(probability, minInliers, maxIterations)      the reference's defaults; the effective mRansacMaxIts comes from hs_sim3_plan
//   iterate(nIterations, bNoMore, vbInliers, nInliers) / find(vbInliers12, nInliers)
//   GetEstimatedRotation() / GetEstimatedTranslation() / GetEstimatedScale()
//
// and one call for all consistent candidates of LoopClosing::ComputeSim3, which the reference runs round-robin:
//
//   HipSim3Solver::iterate(solvers, nIterations, results)      static: ONE hs_sim3_iterate for every solver of the list
//
// The state (mnIterations, the best count, mask and pose) lives in the object and persists across calls as the reference's does.  `seed` replaces
// the process-wide generator all of the reference's solvers share: give every candidate its own.
#pragma once
#ifdef HYSLAM_AMD_WITH_HYSLAM
#include <KeyFrame.h>
#include <MapPoint.h>
#else
#include "cv_compat.h"
#endif
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/hyslam_amd.h"
#include "HipORBExtractor.h"
#include "HipRansacBatch.h"

namespace HYSLAM {

class HipSim3Solver {
public:
    // what one solver's part of a call gave: the arguments iterate() hands back
    struct Result { cv::Mat T12; bool bNoMore = false; std::vector<bool> vbInliers; int nInliers = 0; hs_sim3_result info; };

    HipSim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale = true, uint64_t seed = 0, hs_orb* handle = nullptr)
        : handle_(handle), n_matches_(vpMatched12.size())
    {
        const FeatureViews KF1views = pKF1->getViews();
        const FeatureExtractorSettings orb1 = KF1views.orbParams();
        const FeatureViews KF2views = pKF2->getViews();
        const FeatureExtractorSettings orb2 = KF2views.orbParams();
        const std::vector<MapPoint*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
        const cv::Mat Rcw1 = pKF1->GetRotation(), tcw1 = pKF1->GetTranslation(), Rcw2 = pKF2->GetRotation(), tcw2 = pKF2->GetTranslation();
        for (size_t i1 = 0; i1 < vpMatched12.size(); i1++) {
            MapPoint* pMP2 = vpMatched12[i1];
            if (!pMP2) continue;
            MapPoint* pMP1 = i1 < vpKeyFrameMP1.size() ? vpKeyFrameMP1[i1] : nullptr;
            if (!pMP1) continue;
            if (pMP1->isBad() || pMP2->isBad()) continue;
            const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1), indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (indexKF1 < 0 || indexKF2 < 0) continue;
            hs_sim3_corr c = hs_sim3_corr();
            const float s1 = KF1views.keypt(indexKF1).size / orb1.size_ref, s2 = KF2views.keypt(indexKF2).size / orb2.size_ref;      // determineSigma2, in float
            c.sigma2_1 = orb1.sigma_ref * (s1 * s1); c.sigma2_2 = orb2.sigma_ref * (s2 * s2);
            to_camera(Rcw1, tcw1, pMP1->GetWorldPos(), c.X1c);
            to_camera(Rcw2, tcw2, pMP2->GetWorldPos(), c.X2c);
            c.idx1 = (int32_t)i1;
            corrs_.push_back(c);
        }
        params_ = hs_sim3_params();
        const Camera& c1 = pKF1->getCamera(); const Camera& c2 = pKF2->getCamera();
        params_.fx1 = c1.fx(); params_.fy1 = c1.fy(); params_.cx1 = c1.cx(); params_.cy1 = c1.cy();
        params_.fx2 = c2.fx(); params_.fy2 = c2.fy(); params_.cx2 = c2.cx(); params_.cy2 = c2.cy();
        params_.fix_scale = bFixScale ? 1 : 0; params_.seed = seed;
        hs_sim3_state_init(&state_);
        best_mask_.assign(corrs_.size(), 0);
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        params_.probability = probability; params_.min_inliers = minInliers; params_.max_iterations = maxIterations;
        if (hs_sim3_plan((int)corrs_.size(), &params_, &plan_) != HS_OK) throw std::invalid_argument("HipSim3Solver: bad RANSAC parameters");
        state_.iterations = 0;                                     // mnIterations = 0 (:141)
    }

    cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers) {
        bool bFlag;
        return iterate(plan_.max_iterations, bFlag, vbInliers12, nInliers);
    }

    cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        std::vector<HipSim3Solver*> one(1, this);
        std::vector<Result> r;
        iterate(one, nIterations, r);
        bNoMore = r[0].bNoMore; vbInliers = r[0].vbInliers; nInliers = r[0].nInliers;
        return r[0].T12;
    }

    // iterate(nIterations) of every solver in one call; results[q] belongs to solvers[q].  All solvers run on the first one's handle.
    static void iterate(const std::vector<HipSim3Solver*>& solvers, int nIterations, std::vector<Result>& results) {
        const int Q = (int)solvers.size();
        results.assign(Q, Result());
        const hip_detail::RansacBatch<HipSim3Solver, hs_sim3_result> b(solvers, nIterations, "HipSim3Solver", hs_sim3_iterate);
        for (int q = 0; q < Q; q++) {
            const HipSim3Solver& s = *solvers[q];
            Result& r = results[q];
            r.info = b.res[q];
            r.bNoMore = b.res[q].status == HS_SIM3_TOO_FEW || b.res[q].status == HS_SIM3_EXHAUSTED;
            r.nInliers = b.res[q].n_inliers;
            r.vbInliers.assign(s.n_matches_, false);               // always mN1 long (:147)
            for (int64_t k = b.offsets[q]; k < b.offsets[q + 1]; k++)
                if (b.inliers[(size_t)k]) r.vbInliers[(size_t)b.corrs[(size_t)k].idx1] = true;
            if (b.res[q].status != HS_SIM3_FOUND && b.res[q].status != HS_SIM3_NONFINITE) continue;  // no pose: an empty cv::Mat
            r.T12 = cv::Mat(4, 4, CV_32F);
            for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) r.T12.at<float>(i, j) = b.res[q].T12[4 * i + j];
        }
    }

    cv::Mat GetEstimatedRotation() { cv::Mat R(3, 3, CV_32F); for (int i = 0; i < 9; i++) R.at<float>(i / 3, i % 3) = state_.R[i]; return R; }
    cv::Mat GetEstimatedTranslation() { cv::Mat t(3, 1, CV_32F); for (int i = 0; i < 3; i++) t.at<float>(i) = state_.t[i]; return t; }
    float GetEstimatedScale() { return state_.s; }

    int correspondences() const { return (int)corrs_.size(); }
    const std::vector<hs_sim3_corr>& gathered() const { return corrs_; }
    const hs_sim3_plan_t& plan() const { return plan_; }          // the effective max_iterations and epsilon
    const hs_sim3_state& state() const { return state_; }

private:
    // Rcw * X3Dw + tcw as one product (double accumulation in index order, one narrowing)
    static void to_camera(const cv::Mat& R, const cv::Mat& t, const cv::Mat& X, float* out) {
        for (int i = 0; i < 3; i++)
            out[i] = (float)((((double)R.at<float>(i, 0) * (double)X.at<float>(0) + (double)R.at<float>(i, 1) * (double)X.at<float>(1)) +
                              (double)R.at<float>(i, 2) * (double)X.at<float>(2)) + (double)t.at<float>(i));
    }

    friend struct hip_detail::RansacBatch<HipSim3Solver, hs_sim3_result>;
    hs_orb* handle_;
    size_t n_matches_;
    std::vector<hs_sim3_corr> corrs_;
    hs_sim3_params params_;
    hs_sim3_plan_t plan_;
    hs_sim3_state state_;
    std::vector<uint8_t> best_mask_;
};

}  // namespace HYSLAM
