// kernels_track_initial.hip — the two gates of TrackingStateNormal::initialPoseEstimation (src/slam/tracking/TrackingStateNormal.cpp:21-58) on the
// device, for the composites of hs_track_initial.hip (include/hyslam_amd.h, "initial pose estimation as one resident call"):
//   k_init_gate        `if (nmatches < thresh_init)` (:34) and `if (nmatches < N_min_matches_BoW) return -1` (TrackReferenceKeyFrame.cpp:27) as one
//                      status word, and the search's ops masked by it: with every op at -1 the view-order replay is the identity
//   k_init_edges_gate  what the optimiser sees: no edge unless the stage runs (k_track_gate's mechanism)
//   k_init_finish      the stage's return value, `success` (:41) and the pose the frame holds afterwards
//   k_frame_result     one hs_track_result for the key-frame stage (:41,71 for every path, the fall-back included)
// Integer and flag work only.  No kernel waits on memory another workgroup or a later launch writes; the kernel boundary is the only synchronisation.
#include "hs_track.h"

namespace {
// TrackMotionModel::track's return value as initialPoseEstimation reads it; 0 for a stage that is not predicated on one
__device__ inline int init_motion_return(const hs_track_result* motion)
{
    if (!motion) return 0;
    return motion->status == HS_TRACK_MOTION_FAILED ? -1 : motion->n_matches_map;
}

// every thread reads the same two words and evaluates the same gate; thread 0 records it, thread f masks op f
// (result->n_bow is where the search left its count: it is read here and stays)
__global__ __launch_bounds__(HS_TRACK_BLOCK) void k_init_gate(int n, const hs_track_result* __restrict__ motion, int n_min_matches_bow, int thresh_init,
                                                              const int32_t* __restrict__ op_view, const int32_t* __restrict__ op_lm, int32_t* __restrict__ op_view_run,
                                                              int32_t* __restrict__ op_lm_run, hs_track_initial_result* result)
{
    const int n_bow = result->n_bow;
    const int motion_return = init_motion_return(motion);
    const bool run = !motion || motion_return < thresh_init;
    const int status = !run ? HS_REFKF_SKIPPED : n_bow < n_min_matches_bow ? HS_REFKF_BOW_FAILED : HS_REFKF_OK;
    const int f = blockIdx.x * HS_TRACK_BLOCK + threadIdx.x;
    if (f == 0) result->refkf_status = status;
    if (f < n) {
        const bool ok = status == HS_REFKF_OK;
        op_view_run[f] = ok ? op_view[f] : -1;
        op_lm_run[f] = ok ? op_lm[f] : -1;
    }
}

__global__ void k_init_edges_gate(const hs_track_initial_result* __restrict__ result, int32_t* __restrict__ n_edges)
{
    n_edges[1] = result->refkf_status == HS_REFKF_OK ? n_edges[0] : 0;
}

// result->n_matches_map_refkf holds the discard's count already (0 when the stage did not run: the discard saw no edge)
__global__ void k_init_finish(const hs_track_result* __restrict__ motion, int thresh_init, const hs_pose_result* __restrict__ pose, const uint32_t* __restrict__ Tcw_entry,
                              uint32_t* __restrict__ Tcw_init, hs_track_initial_result* __restrict__ result)
{
    const int status = result->refkf_status;
    const int n_init = status == HS_REFKF_OK ? result->n_matches_map_refkf : status == HS_REFKF_BOW_FAILED ? -1 : init_motion_return(motion);
    result->n_init = n_init;
    result->success = n_init > thresh_init ? 1 : 0;
    for (int i = 0; i < 3; i++) result->_pad[i] = 0;
    const uint32_t* src = status == HS_REFKF_OK ? reinterpret_cast<const uint32_t*>(pose->Tcw) : Tcw_entry;       // as words: the entry pose bit for bit
    for (int i = 0; i < 16; i++) Tcw_init[i] = src[i];
}

__global__ void k_frame_result(const hs_track_result* __restrict__ motion, const hs_track_initial_result* __restrict__ init, const int32_t* __restrict__ n_inliers,
                               hs_track_result* __restrict__ out)
{
    hs_track_result r{};
    r.status = HS_TRACK_OK;
    if (motion) { r.used_wide = motion->used_wide; r.n_narrow = motion->n_narrow; r.n_wide = motion->n_wide; }
    r.n_matches_map = init->n_init;
    r.n_inliers = *n_inliers;
    *out = r;
}
}  // namespace

void hs_launch_init_gate(int n, const hs_track_result* d_motion, const hs_track_refkf_params& rp, const int32_t* d_op_view, const int32_t* d_op_lm,
                         int32_t* d_op_view_run, int32_t* d_op_lm_run, hs_track_initial_result* d_result, hipStream_t s)
{
    hipLaunchKernelGGL(k_init_gate, dim3((unsigned)((std::max(n, 1) + HS_TRACK_BLOCK - 1) / HS_TRACK_BLOCK)), dim3(HS_TRACK_BLOCK), 0, s, n, d_motion,
                       rp.n_min_matches_bow, rp.thresh_init, d_op_view, d_op_lm, d_op_view_run, d_op_lm_run, d_result);
}

void hs_launch_init_edges_gate(const hs_track_initial_result* d_result, int32_t* d_n_edges, hipStream_t s)
{
    hipLaunchKernelGGL(k_init_edges_gate, dim3(1), dim3(1), 0, s, d_result, d_n_edges);
}

void hs_launch_init_finish(const hs_track_result* d_motion, int thresh_init, const hs_pose_result* d_pose, const float* d_Tcw_entry, float* d_Tcw_init,
                           hs_track_initial_result* d_result, hipStream_t s)
{
    hipLaunchKernelGGL(k_init_finish, dim3(1), dim3(1), 0, s, d_motion, thresh_init, d_pose, reinterpret_cast<const uint32_t*>(d_Tcw_entry),
                       reinterpret_cast<uint32_t*>(d_Tcw_init), d_result);
}

void hs_launch_frame_result(const hs_track_result* d_motion, const hs_track_initial_result* d_init, const int32_t* d_n_inliers, hs_track_result* d_out, hipStream_t s)
{
    hipLaunchKernelGGL(k_frame_result, dim3(1), dim3(1), 0, s, d_motion, d_init, d_n_inliers, d_out);
}
