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
        if (Q == 0) return;
        std::vector<hs_pnp_params> params(Q);
        std::vector<int64_t> offsets(Q + 1, 0);
        std::vector<hs_pnp_state> states(Q);
        for (int q = 0; q < Q; q++) {
            params[q] = solvers[q]->params_; states[q] = solvers[q]->state_;
            offsets[q + 1] = offsets[q] + (int64_t)solvers[q]->corrs_.size();
        }
        std::vector<hs_pnp_corr> corrs; std::vector<uint8_t> best;
        corrs.reserve((size_t)offsets[Q]); best.reserve((size_t)offsets[Q]);
        for (int q = 0; q < Q; q++) {
            corrs.insert(corrs.end(), solvers[q]->corrs_.begin(), solvers[q]->corrs_.end());
            best.insert(best.end(), solvers[q]->best_mask_.begin(), solvers[q]->best_mask_.end());
        }
        std::vector<uint8_t> inliers(corrs.size(), 0);
        std::vector<hs_pnp_result> res(Q);
        hs_orb* use = solvers[0]->handle_ ? solvers[0]->handle_ : hip_detail::thread_handle(hip_detail::default_device().load(), "HipPnPsolver");
        const int st = hs_pnp_iterate(use, Q, params.data(), offsets.data(), corrs.data(), nIterations, nullptr, 0, states.data(), best.data(), res.data(), inliers.data());
        if (st != HS_OK) throw std::runtime_error(std::string("HipPnPsolver: ") + hs_status_string(st) + ": " + hs_orb_last_error(use));
        for (int q = 0; q < Q; q++) {
            HipPnPsolver& s = *solvers[q];
            s.state_ = states[q];
            s.best_mask_.assign(best.begin() + offsets[q], best.begin() + offsets[q + 1]);
            Result& r = results[q];
            r.info = res[q];
            r.bNoMore = res[q].status != HS_PNP_REFINED;                                             // HS_PNP_NONFINITE: no pose and bNoMore, also where it replaces REFINED (info keeps the record)
            if (res[q].status != HS_PNP_REFINED && res[q].status != HS_PNP_BEST) continue;           // no pose: vbInliers stays empty, nInliers 0, an empty cv::Mat
            r.nInliers = res[q].n_inliers;
            r.vbInliers.assign(s.n_matches_, false);
            for (int64_t k = offsets[q]; k < offsets[q + 1]; k++)
                if (inliers[(size_t)k]) r.vbInliers[(size_t)corrs[(size_t)k].kp] = true;
            r.Tcw = cv::Mat(4, 4, CV_32F);
            for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) r.Tcw.at<float>(i, j) = res[q].Tcw[4 * i + j];
        }
    }

    int correspondences() const { return (int)corrs_.size(); }
    const hs_pnp_plan_t& plan() const { return plan_; }           // the effective min_inliers, epsilon and max_iterations
    const hs_pnp_state& state() const { return state_; }

private:
    hs_orb* handle_;
    size_t n_matches_;
    std::vector<hs_pnp_corr> corrs_;
    hs_pnp_params params_;
    hs_pnp_plan_t plan_;
    hs_pnp_state state_;
    std::vector<uint8_t> best_mask_;
};

}  // namespace HYSLAM
