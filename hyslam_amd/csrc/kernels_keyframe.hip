// kernels_keyframe.hip — what Tracking::_Track_ does with the frame after the two track functions, on the dense association state (entry points in
// hs_keyframe.hip, include/hyslam_amd.h):
//
//   k_kfd_ref_begin, k_kfd_ref_update   determineReferenceKeyFrame's glue around hs_frame_views / hs_kf_votes     src/main/Tracking.cpp:179-183,273-317
//   k_kfd_gate                          bOK of initialPoseEstimation / refinePoseEstimate                         TrackingStateNormal.cpp:41,71,78-82
//   k_kfd_clean                         HandlePostTrackingSuccess                                                 Tracking.cpp:375-388
//   k_kfd_need                          needNewKeyFrame, KeyFrame::TrackedMapPoints                               TrackingStateNormal.cpp:87-170, KeyFrame.cc:201-222
//   k_kfd_create_keys, k_kfd_create_rank  createNewKeyFrame, Frame::UnprojectStereo                               TrackingState.cpp:20-93, Frame.cc:481-494
//   k_kfd_discard                       the final outlier removal                                                 Tracking.cpp:219-225
//
// Gates are words of *result in HBM that an earlier launch wrote: a kernel reads its flag at entry, writes zeros to its outputs and returns.  Nothing
// waits on another workgroup; the per-view passes are one workgroup (n <= 65535: at most 64 trips), the ranking is one thread per view over all keys.
//
// The depth walk as a closed form.  The sorted list is ascending, so `depth_j > th_depth` is monotone in the position j: with f = the number of
// candidates that are NOT far, position j is far <=> j >= f.  Both branches of the loop increment nPoints, so nPoints = j + 1 after position j and the
// `break` fires at the first j with j >= f && j + 1 > n_min_points, i.e. j* = max(n_min_points, f); it exists when that is below the list length.
// A view is processed <=> its rank < n_processed; every creating view sorted before a processed one is processed too, so the creation number of a
// view is the count of creating views with a smaller key.  key = depth bits << 32 | view << 1 | creates: monotone for positive floats, unique.
#include "hs_track.h"

namespace {
constexpr int KFD_WG = 1024;
constexpr int KFD_RANK = 256;

__global__ void k_kfd_ref_begin(int n, int64_t* q_off) { q_off[0] = 0; q_off[1] = n; }
// `if (mCurrentFrame.mpReferenceKF) mpReferenceKF[cam_cur] = ...` (:181-183) and the fall-back of :229-230
__global__ void k_kfd_ref_update(const int32_t* max_slot, int32_t* ref_slot, hs_keyframe_result* r)
{
    const int m = *max_slot;
    if (m >= 0) *ref_slot = m;
    r->ref_slot = *ref_slot;
}

__global__ void k_kfd_gate(const hs_track_result* tr, int thresh_init, int thresh_refine, int force_loss, int ok_override, hs_keyframe_result* r)
{
    int ok;
    if (ok_override >= 0) ok = ok_override != 0;
    else ok = tr->status == HS_TRACK_OK && tr->n_matches_map > thresh_init && tr->n_inliers > thresh_refine && !force_loss;
    r->ok = ok;
}

__global__ __launch_bounds__(KFD_WG) void k_kfd_clean(int n, int L, int32_t* kp_lm, uint8_t* kp_outl, int32_t* n_matches, int32_t* kp_lm_obs, const int32_t* lm_nobs,
                                                      hs_keyframe_result* r)
{
    __shared__ int s_removed, s_valid;
    if (!r->ok) { if (threadIdx.x == 0) r->n_valid = 0; return; }
    if (threadIdx.x == 0) { s_removed = 0; s_valid = 0; }
    __syncthreads();
    int removed = 0, valid = 0;
    for (int i = threadIdx.x; i < n; i += KFD_WG) {
        const int k = kp_lm[i];
        if (k < 0) continue;
        if ((unsigned)k < (unsigned)L && lm_nobs[k] < 1) { kp_lm[i] = -1; kp_outl[i] = 0; kp_lm_obs[i] = -1; removed++; }      // pMP->Observations() < 1
        else valid += kp_outl[i] != 2;
    }
    if (removed) atomicAdd(&s_removed, removed);
    if (valid) atomicAdd(&s_valid, valid);
    __syncthreads();
    if (threadIdx.x == 0) { r->n_valid = s_valid; if (s_removed) *n_matches -= s_removed; }
}

__global__ __launch_bounds__(KFD_WG) void k_kfd_need(int n, int L, int sensor, const float* depth, const int32_t* kp_lm, const uint8_t* kp_outl, const uint8_t* lm_bad,
                                                     const int32_t* lm_nobs, int kf_n, const int64_t* kf_off, const int32_t* kf_kp_lm, const int32_t* ref_slot,
                                                     const hs_track_result* tr, const hs_keyframe_params p, hs_keyframe_result* r)
{
    __shared__ int s_ref, s_tracked, s_other;
    if (!r->ok) {
        if (threadIdx.x == 0) { r->n_ref_matches = 0; r->n_tracked_close = 0; r->n_nontracked_close = 0; r->insert = 0; }
        return;
    }
    if (threadIdx.x == 0) { s_ref = 0; s_tracked = 0; s_other = 0; }
    __syncthreads();
    int ref = 0, tracked = 0, other = 0;
    const int min_obs = p.n_kfs_in_map <= 2 ? 2 : 3;
    const int s = *ref_slot;
    if ((unsigned)s < (unsigned)kf_n) {                                                  // D15: no key frame, no tracked points
        const int64_t e = kf_off[s + 1];
        for (int64_t j = kf_off[s] + threadIdx.x; j < e; j += KFD_WG) {
            const int lm = kf_kp_lm[j];
            ref += (unsigned)lm < (unsigned)L && !lm_bad[lm] && lm_nobs[lm] >= min_obs;
        }
    }
    if (sensor != 0)
        for (int i = threadIdx.x; i < n; i += KFD_WG) {
            const float z = depth[i];
            if (z > 0.0f && z < p.th_depth) {
                if (kp_lm[i] >= 0 && kp_outl[i] != 2) tracked++;                         // hasAssociation(i) && !isOutlier(i)
                else other++;
            }
        }
    if (ref) atomicAdd(&s_ref, ref);
    if (tracked) atomicAdd(&s_tracked, tracked);
    if (other) atomicAdd(&s_other, other);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int n_tracked = s_tracked, n_other = s_other, inliers = tr ? tr->n_inliers : 0;
    bool insert = false;
    if (p.force || !p.mapping_stopped) {
        const bool need_close = n_tracked < p.min_N_tracked_close && n_other > p.thresh_N_nontracked_close;
        // unsigned int + int in 32 bits, then widened for the comparison with the long unsigned mnId
        const bool max_exceeded = p.frame_id >= (uint64_t)(uint32_t)(p.last_keyframe_id + (uint32_t)p.max_KF_interval);
        const bool min_exceeded = p.frame_id >= (uint64_t)(uint32_t)(p.last_keyframe_id + (uint32_t)p.min_KF_interval);
        const bool lack_close = sensor != 0 && need_close;
        const bool weak = inliers < (p.N_tracked_target - p.N_tracked_variance);
        const bool dire = inliers < (p.N_tracked_target - 2 * p.N_tracked_variance);
        const bool definite = p.force || max_exceeded || dire;
        const bool optional = min_exceeded && (weak || lack_close);
        if (definite || (optional && p.mapping_idle)) insert = (p.mapping_idle || p.force) ? true : p.mapping_queue_length < 3;
    }
    r->n_ref_matches = s_ref; r->n_tracked_close = n_tracked; r->n_nontracked_close = n_other; r->insert = insert ? 1 : 0;
}

__global__ __launch_bounds__(KFD_WG) void k_kfd_create_keys(int n, int L, int sensor, float th_depth, int n_min_points, int new_cap, const float* depth,
                                                            const int32_t* kp_lm, const int32_t* lm_nobs, unsigned long long* keys, int64_t* obs_off, int64_t* desc_off,
                                                            int32_t* lm_index, hs_keyframe_result* r)
{
    __shared__ int s_cand, s_near;
    const bool on = r->ok && r->insert && sensor != 0;
    if (threadIdx.x == 0) { s_cand = 0; s_near = 0; }
    __syncthreads();
    for (int k = threadIdx.x; k <= new_cap; k += KFD_WG) { obs_off[k] = k; desc_off[k] = k; if (k < new_cap) lm_index[k] = -1; }
    int cand = 0, near = 0;
    for (int i = threadIdx.x; i < n; i += KFD_WG) {
        unsigned long long key = 0;
        const float z = on ? depth[i] : 0.0f;
        if (z > 0.0f) {                                                                  // NaN and <= 0 out, +inf in
            const int lm = kp_lm[i];
            const bool creates = lm < 0 || ((unsigned)lm < (unsigned)L && lm_nobs[lm] < 1);
            key = ((unsigned long long)__float_as_uint(z) << 32) | ((unsigned)i << 1) | (creates ? 1u : 0u);
            cand++;
            near += !(z > th_depth);
        }
        keys[i] = key;
    }
    if (cand) atomicAdd(&s_cand, cand);
    if (near) atomicAdd(&s_near, near);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int n_cand = s_cand, f = s_near, j = max(n_min_points, f);
    r->n_candidates = n_cand;
    r->n_processed = (f < n_cand && j < n_cand) ? j + 1 : n_cand;
    r->n_new = 0;
}

// mRwc * x3Dc + mOw as cv::gemm evaluates a 3x3 by 3x1 float product: double products summed left to right from 0, + C in double, one rounding
__device__ __forceinline__ float kfd_gemm3(float a0, float a1, float a2, float b0, float b1, float b2, float c)
{
    double s = 0.0;
    s = __dadd_rn(s, __dmul_rn((double)a0, (double)b0));
    s = __dadd_rn(s, __dmul_rn((double)a1, (double)b1));
    s = __dadd_rn(s, __dmul_rn((double)a2, (double)b2));
    return (float)__dadd_rn(s, (double)c);
}

struct KfdCreateArgs {
    int32_t n, L, new_cap, lms_cap;
    float fx, fy, cx, cy;
    const hs_keypoint* kps; const uint8_t* desc; const float* depth; const hs_pose_view* pv; const unsigned long long* keys;
    int32_t* kp_lm; uint8_t* kp_outl; int32_t* n_matches; int32_t* kp_lm_obs;
    int32_t* new_view; float* new_pos; hs_lm_entry_in* entries; hs_lm_obs* obs; uint8_t* out_desc; int32_t* lm_index; hs_landmark* lms;
    hs_keyframe_result* r;
};

__global__ __launch_bounds__(KFD_RANK) void k_kfd_create_rank(const KfdCreateArgs a)
{
    __shared__ unsigned long long s_keys[KFD_RANK];
    const int n_proc = a.r->n_processed;                                                 // written by k_kfd_create_keys: 0 when the stage is off
    if (n_proc <= 0) return;
    const int tid = threadIdx.x, i = blockIdx.x * KFD_RANK + tid, n = a.n;
    const unsigned long long my = i < n ? a.keys[i] : 0ull;
    int rank = 0, k = 0;
    for (int base = 0; base < n; base += KFD_RANK) {
        s_keys[tid] = base + tid < n ? a.keys[base + tid] : 0ull;
        __syncthreads();
        if (my) {
            const int m = min(KFD_RANK, n - base);
            for (int t = 0; t < m; t++) {
                const unsigned long long o = s_keys[t];
                const int lt = o != 0ull && o < my;
                rank += lt;
                k += lt & (int)(o & 1ull);
            }
        }
        __syncthreads();
    }
    const bool make = my != 0ull && rank < n_proc && (my & 1ull);
    bool was_empty = false;
    if (make) {
        was_empty = a.kp_lm[i] < 0;
        a.kp_lm[i] = a.L + k;                                                            // removeLandMarkAssociation (when held), then the fresh insert
        if (!was_empty || !a.kp_outl[i]) a.kp_outl[i] = 1;                               // insert({i, false}): a stale entry of an empty view stays
        a.kp_lm_obs[i] = 0;
        const hs_pose_view pv = *a.pv;
        const hs_keypoint kp = a.kps[i];
        const float z = a.depth[i];
        const float x = __fmul_rn(__fsub_rn(kp.x, a.cx), __fdiv_rn(z, a.fx));             // Camera::Unproject
        const float y = __fmul_rn(__fsub_rn(kp.y, a.cy), __fdiv_rn(z, a.fy));
        float P[3];
        for (int c = 0; c < 3; c++) P[c] = kfd_gemm3(pv.Rcw[c], pv.Rcw[3 + c], pv.Rcw[6 + c], x, y, z, pv.Ow[c]);
        if (k < a.new_cap) {
            a.new_view[k] = i;
            hs_lm_entry_in e;
            hs_lm_obs o;
            for (int c = 0; c < 3; c++) { a.new_pos[3 * k + c] = P[c]; e.pos[c] = P[c]; e.ref_Ow[c] = pv.Ow[c]; o.Ow[c] = pv.Ow[c]; o.assoc_pos[c] = P[c]; }
            o.fx = a.fx; o.fy = a.fy; o.cx = a.cx; o.cy = a.cy; o.u = kp.x; o.v = kp.y; o.kp_size = kp.size; o.assoc = 1;
            a.entries[k] = e;
            a.obs[k] = o;
            const uint32_t* src = reinterpret_cast<const uint32_t*>(a.desc) + (size_t)i * 8;
            uint32_t* dst = reinterpret_cast<uint32_t*>(a.out_desc) + (size_t)k * 8;
            for (int w = 0; w < 8; w++) dst[w] = src[w];
            a.lm_index[k] = a.L + k;
        }
        if (a.lms && a.L + k < a.lms_cap) {
            hs_landmark* rec = a.lms + a.L + k;
            for (int c = 0; c < 3; c++) rec->pos[c] = P[c];
            rec->assoc_kp = -1; rec->prev_angle = 0.0f; rec->skip = 0;
        }
    }
    // counts only: no position depends on the order these arrive in
    const int c_new = __popcll(__ballot(make)), c_empty = __popcll(__ballot(make && was_empty));
    if ((tid & 63) == 0) { if (c_new) atomicAdd(&a.r->n_new, c_new); if (c_empty) atomicAdd(a.n_matches, c_empty); }
}

__global__ __launch_bounds__(KFD_WG) void k_kfd_discard(int n, int32_t* kp_lm, uint8_t* kp_outl, int32_t* n_matches, int32_t* kp_lm_obs, const hs_keyframe_result* r)
{
    __shared__ int s_removed;
    if (!r->ok) return;
    if (threadIdx.x == 0) s_removed = 0;
    __syncthreads();
    int removed = 0;
    for (int i = threadIdx.x; i < n; i += KFD_WG)
        if (kp_lm[i] >= 0 && kp_outl[i] == 2) { kp_lm[i] = -1; kp_outl[i] = 0; kp_lm_obs[i] = -1; removed++; }
    if (removed) atomicAdd(&s_removed, removed);
    __syncthreads();
    if (threadIdx.x == 0 && s_removed) *n_matches -= s_removed;
}
}  // namespace

void hs_launch_kfd_ref_begin(int n, int64_t* d_q_off, hipStream_t s) { hipLaunchKernelGGL(k_kfd_ref_begin, dim3(1), dim3(1), 0, s, n, d_q_off); }
void hs_launch_kfd_ref_update(const int32_t* d_max_slot, int32_t* d_ref_slot, hs_keyframe_result* d_result, hipStream_t s)
{
    hipLaunchKernelGGL(k_kfd_ref_update, dim3(1), dim3(1), 0, s, d_max_slot, d_ref_slot, d_result);
}
void hs_launch_kfd_gate(const hs_track_result* d_track_result, const hs_keyframe_params& p, hs_keyframe_result* d_result, hipStream_t s)
{
    hipLaunchKernelGGL(k_kfd_gate, dim3(1), dim3(1), 0, s, d_track_result, p.thresh_init, p.thresh_refine, p.force_loss, p.ok_override, d_result);
}
void hs_launch_kfd_clean(int n, const hs_track_state& st, const hs_kf_table& T, hs_keyframe_result* d_result, hipStream_t s)
{
    hipLaunchKernelGGL(k_kfd_clean, dim3(1), dim3(KFD_WG), 0, s, n, T.L, st.kp_lm, st.kp_outl, st.n_matches, st.kp_lm_obs, T.lm_nobs, d_result);
}
void hs_launch_kfd_need(int n, int sensor, const float* d_depth, const hs_track_state& st, const hs_kf_table& T, const hs_kf_features& K, const int32_t* d_ref_slot,
                        const hs_track_result* d_track_result, const hs_keyframe_params& p, hs_keyframe_result* d_result, hipStream_t s)
{
    hipLaunchKernelGGL(k_kfd_need, dim3(1), dim3(KFD_WG), 0, s, n, T.L, sensor, d_depth, st.kp_lm, st.kp_outl, T.lm_bad, T.lm_nobs, K.n_kf, K.kf_off, K.kp_lm, d_ref_slot,
                       d_track_result, p, d_result);
}
void hs_launch_kfd_create(const hs_frame_view& F, const float* d_depth, const hs_track_state& st, const hs_kf_table& T, const hs_keyframe_params& p, int new_cap,
                          const hs_keyframe_out& out, unsigned long long* d_keys, hipStream_t s)
{
    hipLaunchKernelGGL(k_kfd_create_keys, dim3(1), dim3(KFD_WG), 0, s, F.n, T.L, F.sensor, p.th_depth, p.n_min_points, new_cap, d_depth, st.kp_lm, T.lm_nobs, d_keys,
                       out.obs_offsets, out.desc_offsets, out.lm_index, out.result);
    const KfdCreateArgs a{F.n, T.L, new_cap, out.lms ? out.lms_cap : 0, F.fx, F.fy, F.cx, F.cy, F.kps, F.desc, d_depth, out.pose_view, d_keys,
                          st.kp_lm, st.kp_outl, st.n_matches, st.kp_lm_obs, out.new_view, out.new_pos, out.entries, out.obs, out.desc, out.lm_index, out.lms, out.result};
    hipLaunchKernelGGL(k_kfd_create_rank, dim3((unsigned)((F.n + KFD_RANK - 1) / KFD_RANK)), dim3(KFD_RANK), 0, s, a);
}
void hs_launch_kfd_discard(int n, const hs_track_state& st, const hs_keyframe_result* d_result, hipStream_t s)
{
    hipLaunchKernelGGL(k_kfd_discard, dim3(1), dim3(KFD_WG), 0, s, n, st.kp_lm, st.kp_outl, st.n_matches, st.kp_lm_obs, d_result);
}
