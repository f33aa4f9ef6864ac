// HipPoseOptimizer.h — Optimizer::PoseOptimization (src/optimizers/Optimizer.cc:48-279) over the C ABI (hs_pose_optimize, include/hyslam_amd.h):
//
//   HipPoseOptimizer::PoseOptimization(pFrame, optParams)   a drop-in for Optimizer::PoseOptimization at its call sites (TrackMotionModel.cpp:59,
//                                                            TrackLocalMap.cpp:22, TrackReferenceKeyFrame.cpp:34, TrackPlaceRecognition.cpp:133-169)
//
// The adaptor gathers one edge per keypoint that holds a landmark, in keypoint order as the reference builds its edges (:105-188, setOutlier(i, false)
// included), makes ONE host call — four rounds of Levenberg-Marquardt and the classification run inside one kernel launch — and replays
// setOutlier(i, flag) for every edge and SetPose.  With fewer than 3 edges nothing else happens and 0 is returned, as in the reference.  optParams is
// accepted and not read, as in the reference.
#pragma once
#ifdef HYSLAM_AMD_WITH_HYSLAM
#include <Frame.h>
#include <MapPoint.h>
#include <ORBSLAM_datastructs.h>
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

class HipPoseOptimizer {
public:
    // what the last call on this thread did, for callers that want more than the return value
    struct Info { int n_edges = 0, rounds = 0, lm_iterations = 0, lm_trials = 0, status = HS_POSE_TOO_FEW; };

    // the edges of pFrame in keypoint order; `index[k]` is the keypoint of edge k.  Calls pFrame->setOutlier(i, false) as the reference does while it
    // builds its edges.
    static void gatherEdges(Frame* pFrame, std::vector<hs_pose_edge>& edges) {
        edges.clear();
        const int N = pFrame->N;
        const FeatureViews& views = pFrame->getViews();
        const FeatureExtractorSettings orb_params = views.orbParams();
        for (int i = 0; i < N; i++) {
            MapPoint* pMP = pFrame->hasAssociation(i);
            if (!pMP) continue;
            pFrame->setOutlier(i, false);
            const cv::KeyPoint kpUn = views.keypt(i);
            const cv::Mat Xw = pMP->GetWorldPos();
            hs_pose_edge e;
            e.Xw[0] = Xw.at<float>(0); e.Xw[1] = Xw.at<float>(1); e.Xw[2] = Xw.at<float>(2);
            e.u = kpUn.pt.x; e.v = kpUn.pt.y; e.ur = views.uR(i);
            const float scale_factor = kpUn.size / orb_params.size_ref;                    // determineSigma2 (FeatureExtractorSettings.cpp:5-8), in float
            e.inv_sigma2 = 1 / (orb_params.sigma_ref * (scale_factor * scale_factor));
            e.kp = i;
            edges.push_back(e);
        }
    }

    // `handle`: any hs_orb on the device to run on; NULL = the calling thread's handle on hip_detail::default_device()
    static int PoseOptimization(Frame* pFrame, optInfo /*optParams*/, hs_orb* handle = nullptr, Info* info = nullptr) {
        std::vector<hs_pose_edge> edges;
        gatherEdges(pFrame, edges);
        if (info) *info = Info();
        if (info) info->n_edges = (int)edges.size();
        if (edges.size() < 3) return 0;                                                     // if(nInitialCorrespondences<3) return 0;
        hs_pose_problem P;
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) P.Tcw[4 * r + c] = pFrame->mTcw.at<float>(r, c);
        const Camera& camera = pFrame->getCamera();
        P.fx = camera.fx(); P.fy = camera.fy(); P.cx = camera.cx(); P.cy = camera.cy(); P.bf = camera.mbf;
        const int64_t offsets[2] = { 0, (int64_t)edges.size() };
        std::vector<uint8_t> outlier(edges.size(), 0);
        hs_pose_result R;
        hs_orb* use = handle ? handle : hip_detail::thread_handle(hip_detail::default_device().load(), "HipPoseOptimizer");
        const int st = hs_pose_optimize(use, 1, &P, offsets, edges.data(), outlier.data(), &R);
        if (st != HS_OK) throw std::runtime_error(std::string("HipPoseOptimizer: ") + hs_status_string(st) + ": " + hs_orb_last_error(use));
        for (size_t k = 0; k < edges.size(); k++) pFrame->setOutlier(edges[k].kp, outlier[k] != 0);
        cv::Mat pose(4, 4, CV_32F);                                                         // Converter::toCvMat(SE3quat_recov)
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) pose.at<float>(r, c) = R.Tcw[4 * r + c];
        pFrame->SetPose(pose);
        if (info) { info->rounds = R.rounds; info->lm_iterations = R.lm_iterations; info->lm_trials = R.lm_trials; info->status = R.status; }
        return R.n_good;
    }
};

}  // namespace HYSLAM
