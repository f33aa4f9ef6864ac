// HipPnPsolver.h — PnPsolver (src/estimators/PnPsolver.h:61-72) over the C ABI (hs_pnp_iterate, include/hyslam_amd.h): the reference's public surface,
//
//   HipPnPsolver(F, vpMapPointMatches)            gathers the correspondences in keypoint order as the reference's constructor does (:69-116)
//   SetRansacParameters(...)                      the reference's defaults; the effective values come from hs_pnp_plan
//   iterate(nIterations, bNoMore, vbInliers, nInliers) / find(vbInliers, nInliers)
//
// and one call for all candidates of a relocalisation, which the reference runs one after another:
//
//   HipPnPsolver::iterate(solvers, nIterations, results)      static: ONE hs_pnp_iterate for every solver of the list
//
// The state (mnIterations, the best count, mask and pose) lives in the object and persists across calls as the reference's does.  `seed` replaces
// the process-wide rand() stream all of the reference's solvers share: give every candidate its own.
#pragma once
#ifdef HYSLAM_AMD_WITH_HYSLAM
#include <Frame.h>
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

class HipPnPsolver {
public:
    // what one solver's part of a call gave: the arguments iterate() hands back
    struct Result { cv::Mat Tcw; bool bNoMore = true; std::vector<bool> vbInliers; int nInliers = 0; hs_pnp_result info; };

    HipPnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches, uint64_t seed = 0, hs_orb* handle = nullptr)
        : handle_(handle), n_matches_(vpMapPointMatches.size())
    {
        const FeatureViews& views = F.getViews();
        const FeatureExtractorSettings orb_params = views.orbParams();
        for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
            MapPoint* pMP = vpMapPointMatches[i];
            if (!pMP || pMP->isBad()) continue;
            const cv::KeyPoint kp = views.keypt(i);
            const cv::Mat Pos = pMP->GetWorldPos();
            hs_pnp_corr c;
            c.Xw[0] = Pos.at<float>(0); c.Xw[1] = Pos.at<float>(1); c.Xw[2] = Pos.at<float>(2);
            c.u = kp.pt.x; c.v = kp.pt.y;
            const float scale_factor = kp.size / orb_params.size_ref;                      // determineSigma2 (FeatureExtractorSettings.cpp:5-8), in float
            c.sigma2 = orb_params.sigma_ref * (scale_factor * scale_factor);
            c.kp = (int32_t)i; c._pad = 0;
            corrs_.push_back(c);
        }
        const Camera& camera = F.getCamera();
        params_.fx = camera.fx(); params_.fy = camera.fy(); params_.cx = camera.cx(); params_.cy = camera.cy();
        params_._pad = 0; params_.seed = seed;
        hs_pnp_state_init(&state_);
        best_mask_.assign(corrs_.size(), 0);
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4, float th2 = 5.991) {
        params_.probability = probability; params_.min_inliers = minInliers; params_.max_iterations = maxIterations; params_.min_set = minSet;
        params_.epsilon = epsilon; params_.th2 = th2;
        if (hs_pnp_plan((int)corrs_.size(), &params_, &plan_) != HS_OK) throw std::invalid_argument("HipPnPsolver: bad RANSAC parameters (minSet < 4)");
    }

    cv::Mat find(std::vector<bool>& vbInliers, int& nInliers) {
        bool bFlag;
        return iterate(plan_.max_iterations, bFlag, vbInliers, nInliers);
    }

    cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        std::vector<HipPnPsolver*> one(1, this);
        std::vector<Result> r;
        iterate(one, nIterations, r);
        bNoMore = r[0].bNoMore; vbInliers = r[0].vbInliers; nInliers = r[0].nInliers;
        return r[0].Tcw;
    }

    // iterate(nIterations) of every solver in one call; results[q] belongs to solvers[q].  All solvers run on the first one's handle.
    static void iterate(const std::vector<HipPnPsolver*>& solvers, int nIterations, std::vector<Result>& results) {
        const int Q = (int)solvers.size();
        results.assign(Q, Result());
        const hip_detail::RansacBatch<HipPnPsolver, hs_pnp_result> b(solvers, nIterations, "HipPnPsolver", hs_pnp_iterate);
        for (int q = 0; q < Q; q++) {
            const HipPnPsolver& s = *solvers[q];
            Result& r = results[q];
            r.info = b.res[q];
            r.bNoMore = b.res[q].status != HS_PNP_REFINED;                                           // HS_PNP_NONFINITE: no pose and bNoMore, also where it replaces REFINED (info keeps the record)
            if (b.res[q].status != HS_PNP_REFINED && b.res[q].status != HS_PNP_BEST) continue;       // no pose: vbInliers stays empty, nInliers 0, an empty cv::Mat
            r.nInliers = b.res[q].n_inliers;
            r.vbInliers.assign(s.n_matches_, false);
            for (int64_t k = b.offsets[q]; k < b.offsets[q + 1]; k++)
                if (b.inliers[(size_t)k]) r.vbInliers[(size_t)b.corrs[(size_t)k].kp] = true;
            r.Tcw = cv::Mat(4, 4, CV_32F);
            for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) r.Tcw.at<float>(i, j) = b.res[q].Tcw[4 * i + j];
        }
    }

    int correspondences() const { return (int)corrs_.size(); }
    const hs_pnp_plan_t& plan() const { return plan_; }           // the effective min_inliers, epsilon and max_iterations
    const hs_pnp_state& state() const { return state_; }

private:
    friend struct hip_detail::RansacBatch<HipPnPsolver, hs_pnp_result>;
    hs_orb* handle_;
    size_t n_matches_;
    std::vector<hs_pnp_corr> corrs_;
    hs_pnp_params params_;
    hs_pnp_plan_t plan_;
    hs_pnp_state state_;
    std::vector<uint8_t> best_mask_;
};

}  // namespace HYSLAM
