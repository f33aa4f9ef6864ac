// HipRansacBatch.h — what the static batched forms of HipPnPsolver, HipSim3Solver and HipMonoEstimator share (the handle and the error of one call
// for all: batch_handle, batch_check) and what the static iterate(solvers, nIterations, results) of the first two share: gather every solver's parameters,
// state, correspondences and best mask into the flat arrays of hs_pnp_iterate / hs_sim3_iterate (include/hyslam_amd.h), make ONE call on the first
// solver's handle, and put every solver's state and best mask back.  What a status means, and the Result it becomes, stays with each solver.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>
#include "HipORBExtractor.h"

namespace HYSLAM {
namespace hip_detail {

// the handle a batched call runs on (the first solver's, or the calling thread's own) and the exception a failed call becomes: shared by RansacBatch
// below and by HipMonoEstimator's static Initialize, whose call has no state and therefore no RansacBatch
inline hs_orb* batch_handle(hs_orb* first, const char* who) { return first ? first : thread_handle(default_device().load(), who); }
inline void batch_check(int st, hs_orb* use, const char* who) {
    if (st != HS_OK) throw std::runtime_error(std::string(who) + ": " + hs_status_string(st) + ": " + hs_orb_last_error(use));
}

// Solver has handle_, params_, state_, corrs_ and best_mask_ (and names this struct a friend); Info is the hs_*_result of its C entry point `iterate`.
// After construction offsets, corrs, inliers and res hold the call's arrays: solver q owns [offsets[q], offsets[q + 1]) of corrs and inliers.
template <class Solver, class Info> struct RansacBatch {
    std::vector<int64_t> offsets;
    std::vector<typename decltype(Solver::corrs_)::value_type> corrs;
    std::vector<uint8_t> inliers;
    std::vector<Info> res;

    template <class Iterate> RansacBatch(const std::vector<Solver*>& solvers, int nIterations, const char* who, Iterate iterate) {
        const int Q = (int)solvers.size();
        if (Q == 0) return;
        std::vector<decltype(Solver::params_)> params(Q);
        std::vector<decltype(Solver::state_)> states(Q);
        offsets.assign(Q + 1, 0);
        for (int q = 0; q < Q; q++) {
            params[q] = solvers[q]->params_; states[q] = solvers[q]->state_;
            offsets[q + 1] = offsets[q] + (int64_t)solvers[q]->corrs_.size();
        }
        std::vector<uint8_t> best;
        corrs.reserve((size_t)offsets[Q]); best.reserve((size_t)offsets[Q]);
        for (int q = 0; q < Q; q++) {
            corrs.insert(corrs.end(), solvers[q]->corrs_.begin(), solvers[q]->corrs_.end());
            best.insert(best.end(), solvers[q]->best_mask_.begin(), solvers[q]->best_mask_.end());
        }
        // No spare element: where no solver has a correspondence the three vectors are empty and their data() may be null, which both entry points
        // accept — they ask for corrs and the two masks only where corr_offsets[Q] > 0, and stage, copy and index nothing of an empty array.
        inliers.assign(corrs.size(), 0);
        res.resize(Q);
        hs_orb* use = batch_handle(solvers[0]->handle_, who);
        const int st = iterate(use, Q, params.data(), offsets.data(), corrs.data(), nIterations, nullptr, 0, states.data(), best.data(), res.data(), inliers.data());
        batch_check(st, use, who);
        for (int q = 0; q < Q; q++) {
            solvers[q]->state_ = states[q];
            solvers[q]->best_mask_.assign(best.begin() + offsets[q], best.begin() + offsets[q + 1]);
        }
    }
};

}  // namespace hip_detail
}  // namespace HYSLAM
