// hs_poseopt.hip — entry points of the pose-only optimisation (include/hyslam_amd.h): hs_pose_optimize(_device), hs_pose_work_bytes and
// hs_pose_edges_device.  The kernels and their launchers are in kernels_poseopt.hip.  The host form checks its arguments and stages through HsStage;
// the device forms check nothing that lives on the device and claim nothing of the handle's scratch, so a chain of launches never waits for it.
#include "hs_track.h"               // the predicates of the two device forms, which the track stages call too

extern "C" {

// both kernels keep their temporaries in registers and LDS
size_t hs_pose_work_bytes(int Q, int64_t n_edges_total) { (void)Q; (void)n_edges_total; return 0; }

int hs_pose_optimize_device(hs_orb* h, int Q, const hs_pose_problem* d_problems, const int64_t* d_edge_offsets, const int32_t* d_n_edges, int edge_cap,
                            const hs_pose_edge* d_edges, uint8_t* d_outlier, hs_pose_result* d_results, void* d_work, void* stream)
{
    (void)d_work;
    return hs_device_call(h, hs_pose_optimize_why(Q, d_problems, d_edge_offsets, d_n_edges, edge_cap, d_edges, d_results), stream,
                          [&](hipStream_t s) { hs_launch_pose_optimize(Q, d_problems, d_edge_offsets, d_n_edges, edge_cap, d_edges, d_outlier, d_results, s); });
}

int hs_pose_optimize(hs_orb* h, int Q, const hs_pose_problem* problems, const int64_t* edge_offsets, const hs_pose_edge* edges, uint8_t* outlier,
                     hs_pose_result* results)
{
    if (!h) return HS_ERR_INVALID;
    if (Q < 0 || !edge_offsets || (Q > 0 && (!problems || !results))) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (!hs_csr_ok(edge_offsets, Q)) return hs_fail(h, HS_ERR_INVALID, "offsets must be non-negative and non-decreasing");
    const size_t n_total = (size_t)edge_offsets[Q];
    if (n_total > 0 && (!edges || !outlier)) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (Q == 0) return HS_OK;
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    HsStage st(h);
    hs_pose_problem* d_prob; int64_t* d_off; hs_pose_edge* d_edges; uint8_t* d_out; hs_pose_result* d_res;
    st.in(&d_prob, (size_t)Q, problems); st.in(&d_off, (size_t)Q + 1, edge_offsets); st.in(&d_edges, n_total, edges);
    st.inout(&d_out, n_total, outlier);                            // the flags of a problem that does not run come back as they went
    st.out(&d_res, (size_t)Q, results);
    const int rc = st.begin();
    if (rc != HS_OK) return rc;
    hs_launch_pose_optimize(Q, d_prob, d_off, nullptr, 0, d_edges, d_out, d_res, st.stream());
    return st.finish();
}

int hs_pose_edges_device(hs_orb* h, const hs_frame_view* F, const hs_landmark* d_lms, int L, const int32_t* d_kp_lm, float sigma_ref,
                         hs_pose_edge* d_edges, int cap, int32_t* d_n_edges, void* d_work, void* stream)
{
    (void)d_work;
    return hs_device_call(h, hs_pose_edges_why(F, d_lms, L, d_kp_lm, d_edges, cap, d_n_edges), stream,
                          [&](hipStream_t s) { hs_launch_pose_edges(*F, d_lms, L, d_kp_lm, sigma_ref, d_edges, cap, d_n_edges, s); });
}

}  // extern "C"
