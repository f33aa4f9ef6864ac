// kernels_track.hip — the glue of the resident per-frame tracking chain (entry points in hs_track.hip, include/hyslam_amd.h):
//
//   k_pose_view            Frame::SetPose / UpdatePoseMatrices                              src/core/Frame.cc
//   k_assoc_*              the association loop of _SearchByProjection_ as a closed form    src/features/FeatureMatcher.cc:113-118,
//                                                                                           src/core/LandMarkMatches.cpp:26-51
//   k_frame_views          kp_lm_obs + removeLandMarkAssociation of bad landmarks           src/slam/tracking/TrackLocalMap.cpp:56-67
//   k_track_discard        the loops after PoseOptimization                                 TrackMotionModel.cpp:62-79, TrackLocalMap.cpp:25-38
//   k_last_gather, k_track_clear, k_track_select, k_track_gate                              TrackMotionModel.cpp:35-56
//
// The replay.  Ops are applied in ascending landmark index and every landmark has at most one op, so "op k" names the op of
// landmark k and "time k" the moment it runs.  Only op k ever writes or erases landmark k.  With kp0 = the state before the replay and, per view u,
// minw[u] / maxw[u] = the smallest / largest landmark among the ops that target u (none: INT_MAX / -1):
//   * u still holds kp0[u] = k at time k  <=>  no earlier op wrote u  <=>  minw[u] >= k   (nothing but op k erases a holder of k)
//   * hasAssociation(k) at time k = jk[k] = the lowest such u; op k erases view jk[k] when it is not its own view
//   * an erased view u had minw[u] > kp0[u]: it is empty when its first op (if any) runs
//   * the last op of a view decides its landmark: no later op can erase it (that op's landmark would have to be kp0[u] > maxw[u] >= minw[u])
//   * the first op of view v (landmark minw[v]) is the fresh insert <=> v is empty then (kp0[v] < 0 or erased) and jk[minw[v]] is none; every
//     other op is a "replace" call, which sets outliers[v] = false
// Four phases with a kernel boundary between them (ops -> views -> ops -> views); integer atomicMin / atomicMax only.
#include "hs_track.h"

namespace {
constexpr int TRK_NONE = 0x7FFFFFFF;

__device__ __forceinline__ float trk_gemm3(float a0, float a1, float a2, float b0, float b1, float b2, float c, double alpha)
{
    double s = 0.0;
    s = __dadd_rn(s, __dmul_rn((double)a0, (double)b0));
    s = __dadd_rn(s, __dmul_rn((double)a1, (double)b1));
    s = __dadd_rn(s, __dmul_rn((double)a2, (double)b2));
    return (float)__dadd_rn(__dmul_rn(alpha, s), (double)c);
}

// one thread: the pose view and, for the optimiser, the problem (the pose with the camera beside it)
// alpha (-1) is an ARGUMENT, as it is one of cv::gemm: a literal would let the compiler turn the product into a negation, which flips the sign of a
// NaN where the multiplication keeps it
__global__ void k_pose_view(const float* __restrict__ Tcw, hs_pose_view* __restrict__ out, hs_pose_problem* __restrict__ prob, float fx, float fy, float cx,
                            float cy, float bf, double alpha)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float T[16];
    for (int i = 0; i < 16; i++) T[i] = Tcw[i];
    hs_pose_view V;
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) V.Rcw[3 * r + c] = T[4 * r + c]; V.tcw[r] = T[4 * r + 3]; }
    for (int i = 0; i < 3; i++) V.Ow[i] = trk_gemm3(T[i], T[4 + i], T[8 + i], T[3], T[7], T[11], 0.0f, alpha);      // mOw = -mRcw.t() * mtcw
    V._pad = 0.0f;
    *out = V;
    if (prob) { for (int i = 0; i < 16; i++) prob->Tcw[i] = T[i]; prob->fx = fx; prob->fy = fy; prob->cx = cx; prob->cy = cy; prob->bf = bf; }
}

// ---- the replay.  work: minw [n], maxw [n], erased [n] (int32), jk [L]
__global__ __launch_bounds__(HS_TRACK_BLOCK) void k_assoc_init(int n, int L, const int32_t* __restrict__ kp_lm, int n_ops, const int32_t* __restrict__ op_lm,
                                                               int32_t* __restrict__ minw, int32_t* __restrict__ maxw, int32_t* __restrict__ erased, int32_t* __restrict__ jk)
{
    const int t = blockIdx.x * HS_TRACK_BLOCK + threadIdx.x;
    if (t < n) {
        minw[t] = TRK_NONE; maxw[t] = -1; erased[t] = 0;
        const int k = kp_lm[t];
        if ((unsigned)k < (unsigned)L) jk[k] = TRK_NONE;
    }
    if (t < n_ops) { const int k = op_lm[t]; if ((unsigned)k < (unsigned)L) jk[k] = TRK_NONE; }
}
__device__ __forceinline__ bool op_valid(int v, int k, int n, int L) { return (unsigned)v < (unsigned)n && (unsigned)k < (unsigned)L; }
__global__ __launch_bounds__(HS_TRACK_BLOCK) void k_assoc_writers(int n, int L, int n_ops, const int32_t* __restrict__ op_view, const int32_t* __restrict__ op_lm,
                                                                  int32_t* __restrict__ minw, int32_t* __restrict__ maxw)
{
    const int j = blockIdx.x * HS_TRACK_BLOCK + threadIdx.x;
    if (j >= n_ops) return;
    const int v = op_view[j], k = op_lm[j];
    if (!op_valid(v, k, n, L)) return;
    atomicMin(&minw[v], k); atomicMax(&maxw[v], k);
}
__global__ __launch_bounds__(HS_TRACK_BLOCK) void k_assoc_holders(int n, int L, const int32_t* __restrict__ kp_lm, const int32_t* __restrict__ minw, int32_t* __restrict__ jk)
{
    const int u = blockIdx.x * HS_TRACK_BLOCK + threadIdx.x;
    if (u >= n) return;
    const int k = kp_lm[u];
    if ((unsigned)k < (unsigned)L && minw[u] >= k) atomicMin(&jk[k], u);
}
__global__ __launch_bounds__(HS_TRACK_BLOCK) void k_assoc_erase(int n, int L, int n_ops, const int32_t* __restrict__ op_view, const int32_t* __restrict__ op_lm,
                                                                const int32_t* __restrict__ jk, int32_t* __restrict__ erased)
{
    const int j = blockIdx.x * HS_TRACK_BLOCK + threadIdx.x;
    if (j >= n_ops) return;
    const int v = op_view[j], k = op_lm[j];
    if (!op_valid(v, k, n, L)) return;
    const int u = jk[k];
    if (u != TRK_NONE && u != v) erased[u] = 1;                 // views_to_landmarks.erase(idx_old): its outliers entry stays, n_matches too
}
__global__ __launch_bounds__(HS_TRACK_BLOCK) void k_assoc_final(int n, int L, int32_t* __restrict__ kp_lm, uint8_t* __restrict__ kp_outl, int32_t* __restrict__ n_matches,
                                                                const int32_t* __restrict__ minw, const int32_t* __restrict__ maxw, const int32_t* __restrict__ erased,
                                                                const int32_t* __restrict__ jk)
{
    const int v = blockIdx.x * HS_TRACK_BLOCK + threadIdx.x;
    bool fresh = false;
    if (v < n) {
        const int first = minw[v], last = maxw[v];
        if (last >= 0) {
            fresh = (kp_lm[v] < 0 || erased[v]) && jk[first] == TRK_NONE;
            kp_lm[v] = last;
            if (!(fresh && first == last && kp_outl[v])) kp_outl[v] = 1;      // insert({i, false}) keeps a stale entry; every replace call sets false
        } else if (erased[v]) kp_lm[v] = -1;
    }
    const int c = __popcll(__ballot(fresh));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(n_matches, c);
}

// ---- per-view passes of one workgroup (n <= 65535: at most 64 trips)
__global__ __launch_bounds__(1024) void k_frame_views(int n, int L, int32_t* __restrict__ kp_lm, uint8_t* __restrict__ kp_outl, int32_t* __restrict__ n_matches,
                                                      const uint8_t* __restrict__ lm_bad, const int32_t* __restrict__ lm_nobs, int drop_bad, int32_t* __restrict__ kp_lm_obs)
{
    __shared__ int dropped;
    if (threadIdx.x == 0) dropped = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        int k = kp_lm[i];
        if (drop_bad && (unsigned)k < (unsigned)L && lm_bad[k]) { kp_lm[i] = k = -1; kp_outl[i] = 0; mine++; }
        kp_lm_obs[i] = (unsigned)k < (unsigned)L ? lm_nobs[k] : -1;
    }
    if (mine) atomicAdd(&dropped, mine);
    __syncthreads();
    if (threadIdx.x == 0 && dropped) *n_matches -= dropped;
}

__global__ __launch_bounds__(1024) void k_track_discard(int mode, const hs_pose_edge* __restrict__ edges, const int32_t* __restrict__ n_edges, int edge_cap,
                                                        const uint8_t* __restrict__ outlier, const hs_pose_result* __restrict__ result, int L,
                                                        const int32_t* __restrict__ lm_nobs, int sensor, int n, int32_t* __restrict__ kp_lm,
                                                        uint8_t* __restrict__ kp_outl, int32_t* __restrict__ n_matches, int32_t* __restrict__ counts)
{
    __shared__ int s_count, s_removed;
    if (threadIdx.x == 0) { s_count = 0; s_removed = 0; }
    __syncthreads();
    const int ne = min(max(*n_edges, 0), edge_cap);
    const bool ran = result->status != HS_POSE_TOO_FEW;
    int count = 0, removed = 0;
    for (int k = threadIdx.x; k < ne; k += 1024) {
        const int i = edges[k].kp;
        if ((unsigned)i >= (unsigned)n) continue;
        if (ran && kp_outl[i]) kp_outl[i] = outlier[k] ? 2 : 1;                     // pFrame->setOutlier(idx, ...): nothing without an `outliers` entry
        const int lm = kp_lm[i];
        if (lm < 0) continue;                                                       // the loop walks the associations: `if(!pMP){continue;}`
        const bool is_out = kp_outl[i] == 2;                                        // isOutlier(LMid)
        if (is_out) {
            if (mode == HS_TRACK_MOTION || sensor == 1) { kp_lm[i] = -1; kp_outl[i] = 0; removed++; }      // removeLandMarkAssociation
        } else if ((unsigned)lm < (unsigned)L && lm_nobs[lm] > 0) count++;
    }
    if (count) atomicAdd(&s_count, count);
    if (removed) atomicAdd(&s_removed, removed);
    __syncthreads();
    if (threadIdx.x == 0) { counts[0] = s_count; if (s_removed) *n_matches -= s_removed; }
}

// ---- TrackMotionModel's own steps
// record j = the landmark of last-frame keypoint j, five lanes per record as k_landmark_gather; piece 2 holds normal[2], assoc_kp, prev_angle, skip
__global__ __launch_bounds__(256) void k_last_gather(const uint4* __restrict__ lms, int L, const int32_t* __restrict__ last_kp_lm, const hs_keypoint* __restrict__ last_kps,
                                                     int n_last, uint4* __restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t j = t / 5;
    const int piece = (int)(t - j * 5);
    if (j >= n_last) return;
    const int src = last_kp_lm[j];
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if ((unsigned)src < (unsigned)L) {
        v = lms[(int64_t)src * 5 + piece];
        if (piece == 2) { v.y = 0xFFFFFFFFu; v.z = __float_as_uint(last_kps[j].angle); v.w = 0u; }
    } else if (piece == 2) { v.y = 0xFFFFFFFFu; v.w = 1u; }
    out[j * 5 + piece] = v;
}
// clearAssociations
__global__ __launch_bounds__(HS_TRACK_BLOCK) void k_track_clear(int n, int32_t* __restrict__ kp_lm, uint8_t* __restrict__ kp_outl, int32_t* __restrict__ n_matches,
                                                                int32_t* __restrict__ kp_lm_obs)
{
    const int i = blockIdx.x * HS_TRACK_BLOCK + threadIdx.x;
    if (i < n) { kp_lm[i] = -1; kp_outl[i] = 0; kp_lm_obs[i] = -1; }
    if (i == 0) *n_matches = 0;
}
// `if (nmatches < N_min_matches) { wider window }` and `if (nmatches < N_min_matches) return -1`: the decision is one thread's, the copy of the
// chosen matches everybody's (the counts are uniform loads)
__global__ __launch_bounds__(HS_TRACK_BLOCK) void k_track_select(int n_last, const int32_t* __restrict__ narrow_idx, const int32_t* __restrict__ narrow_n,
                                                                 const int32_t* __restrict__ wide_idx, const int32_t* __restrict__ wide_n, int n_min_matches,
                                                                 int32_t* __restrict__ op_view, hs_track_result* __restrict__ result)
{
    const int nn = *narrow_n, nw = *wide_n;
    const bool wide = nn < n_min_matches;
    const int j = blockIdx.x * HS_TRACK_BLOCK + threadIdx.x;
    if (j < n_last) op_view[j] = wide ? wide_idx[j] : narrow_idx[j];
    if (j == 0) {
        hs_track_result r{};
        r.status = (wide ? nw : nn) < n_min_matches ? HS_TRACK_MOTION_FAILED : HS_TRACK_OK;
        r.used_wide = wide; r.n_narrow = nn; r.n_wide = nw;
        *result = r;
    }
}
// the optimiser of a failed stage sees no edge
__global__ void k_track_gate(const hs_track_result* __restrict__ result, int32_t* __restrict__ n_edges) { n_edges[1] = result->status == HS_TRACK_MOTION_FAILED ? 0 : n_edges[0]; }
}  // namespace

static dim3 trk_grid(int n) { return dim3((unsigned)((std::max(n, 1) + HS_TRACK_BLOCK - 1) / HS_TRACK_BLOCK)); }

void hs_launch_pose_view(const float* d_Tcw, hs_pose_view* d_out, hs_pose_problem* d_problem, const hs_frame_view* F, hipStream_t s)
{
    hipLaunchKernelGGL(k_pose_view, dim3(1), dim3(64), 0, s, d_Tcw, d_out, d_problem, F ? F->fx : 0.f, F ? F->fy : 0.f, F ? F->cx : 0.f, F ? F->cy : 0.f, F ? F->mbf : 0.f, -1.0);
}

void hs_launch_frame_associate(int n, int L, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, int n_ops, const int32_t* d_op_view, const int32_t* d_op_lm,
                               const HsAssocWork& w, hipStream_t s)
{
    if (n <= 0 || n_ops <= 0) return;
    int32_t *minw = w.minw, *maxw = w.maxw, *erased = w.erased, *jk = w.jk;
    hipLaunchKernelGGL(k_assoc_init, trk_grid(std::max(n, n_ops)), dim3(HS_TRACK_BLOCK), 0, s, n, L, d_kp_lm, n_ops, d_op_lm, minw, maxw, erased, jk);
    hipLaunchKernelGGL(k_assoc_writers, trk_grid(n_ops), dim3(HS_TRACK_BLOCK), 0, s, n, L, n_ops, d_op_view, d_op_lm, minw, maxw);
    hipLaunchKernelGGL(k_assoc_holders, trk_grid(n), dim3(HS_TRACK_BLOCK), 0, s, n, L, d_kp_lm, minw, jk);
    hipLaunchKernelGGL(k_assoc_erase, trk_grid(n_ops), dim3(HS_TRACK_BLOCK), 0, s, n, L, n_ops, d_op_view, d_op_lm, jk, erased);
    hipLaunchKernelGGL(k_assoc_final, trk_grid(n), dim3(HS_TRACK_BLOCK), 0, s, n, L, d_kp_lm, d_kp_outl, d_n_matches, minw, maxw, erased, jk);
}

void hs_launch_frame_views(int n, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, const hs_kf_table& T, int drop_bad, int32_t* d_kp_lm_obs, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_frame_views, dim3(1), dim3(1024), 0, s, n, T.L, d_kp_lm, d_kp_outl, d_n_matches, T.lm_bad, T.lm_nobs, drop_bad, d_kp_lm_obs);
}

void hs_launch_track_discard(int mode, const hs_pose_edge* d_edges, const int32_t* d_n_edges, int edge_cap, const uint8_t* d_outlier, const hs_pose_result* d_result,
                             const hs_kf_table& T, int sensor, int n, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, int32_t* d_counts, hipStream_t s)
{
    hipLaunchKernelGGL(k_track_discard, dim3(1), dim3(1024), 0, s, mode, d_edges, d_n_edges, edge_cap, d_outlier, d_result, T.L, T.lm_nobs, sensor, n, d_kp_lm, d_kp_outl,
                       d_n_matches, d_counts);
}

void hs_launch_last_gather(const hs_landmark* d_lms, int L, const int32_t* d_last_kp_lm, const hs_keypoint* d_last_kps, int n_last, hs_landmark* d_out, hipStream_t s)
{
    const int64_t threads = (int64_t)n_last * 5;
    if (threads <= 0) return;
    hipLaunchKernelGGL(k_last_gather, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const uint4*>(d_lms), L, d_last_kp_lm, d_last_kps, n_last,
                       reinterpret_cast<uint4*>(d_out));
}

void hs_launch_track_clear(int n, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, int32_t* d_kp_lm_obs, hipStream_t s)
{
    hipLaunchKernelGGL(k_track_clear, trk_grid(n), dim3(HS_TRACK_BLOCK), 0, s, n, d_kp_lm, d_kp_outl, d_n_matches, d_kp_lm_obs);
}

void hs_launch_track_select(int n_last, const int32_t* d_narrow_idx, const int32_t* d_narrow_n, const int32_t* d_wide_idx, const int32_t* d_wide_n, int n_min_matches,
                            int32_t* d_op_view, hs_track_result* d_result, hipStream_t s)
{
    hipLaunchKernelGGL(k_track_select, trk_grid(n_last), dim3(HS_TRACK_BLOCK), 0, s, n_last, d_narrow_idx, d_narrow_n, d_wide_idx, d_wide_n, n_min_matches, d_op_view, d_result);
}

void hs_launch_track_gate(const hs_track_result* d_result, int32_t* d_n_edges, hipStream_t s) { hipLaunchKernelGGL(k_track_gate, dim3(1), dim3(1), 0, s, d_result, d_n_edges); }
