// hs_poseopt.h — the pose-only optimisation (Optimizer::PoseOptimization, src/optimizers/Optimizer.cc:48-279): launchers of kernels_poseopt.hip for the
// entry points in hs_poseopt.hip (include/hyslam_amd.h).  All asynchronous on `s`; every pointer is device memory.
#pragma once
#include "hs_internal.h"

#ifndef HS_POSE_THREADS            // k_pose_optimize: one workgroup of four waves per problem; 64 .. 1024 in steps of 64 for the measurement builds
                                   // (the kernel holds 282 VGPRs: from 512 threads up a wave's budget is 256, then 128, and the build spills to scratch)
#define HS_POSE_THREADS 256        // (make BUILD=_build_po128 OUT=../libhyslam_amd_po128.so EXTRA=-DHS_POSE_THREADS=128)
#endif
static_assert(HS_POSE_THREADS % 64 == 0 && HS_POSE_THREADS >= 64 && HS_POSE_THREADS <= 1024, "whole waves");

// one workgroup per problem; exactly one of d_edge_offsets [Q + 1] and d_n_edges [1] (Q == 1: the problem's edges are d_edges[0, min(*d_n_edges, edge_cap)))
void hs_launch_pose_optimize(int Q, const hs_pose_problem* d_problems, const int64_t* d_edge_offsets, const int32_t* d_n_edges, int edge_cap,
                             const hs_pose_edge* d_edges, uint8_t* d_outlier, hs_pose_result* d_results, hipStream_t s);
// F's pointers are device memory (kps, uR; uR == nullptr: every edge is monocular)
void hs_launch_pose_edges(const hs_frame_view& F, const hs_landmark* d_lms, int L, const int32_t* d_kp_lm, float sigma_ref, hs_pose_edge* d_edges, int cap,
                          int32_t* d_n_edges, hipStream_t s);
