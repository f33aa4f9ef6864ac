// hs_localmap.hip — entry points of the local map (include/hyslam_amd.h): hs_local_keyframes(_device), hs_local_points(_device),
// hs_landmark_gather_device and hs_local_map_search_device, which is the vote of hs_kfgraph.hip, these three and the projection search enqueued on one
// stream.  The kernels and their launchers are in kernels_localmap.hip.  The host forms check their arguments and stage through HsStage; the device
// forms take their temporaries from the caller, so nothing here claims the handle's scratch between two launches of a chain.
#include "hs_track.h"

// the vote (keyframeCounter with the bad key frames in it, pKFmax among those that are not bad; no ordered list: TrackLocalMap.cpp:80-123), the local
// key frames, the local points, the gather and the search on one stream
const char* hs_local_map_search_why(const hs_kf_table* T, const int32_t* d_frame_lm, int n_assoc, const int32_t* d_neigh, int neigh_cap, const int32_t* d_parent,
                                    const hs_frame_view* F, const hs_landmark* d_lms, const hs_proj_params* pp, int cap, const hs_local_map_out* out,
                                    const HsLocalMapWork& w)
{
    if (!T || !out || !w.base || cap < 1 || n_assoc < 0 || !out->weights || !out->max_slot || !out->max_count || !out->local || !out->n_local ||
        !out->frame_remove || !out->sel || !out->n_sel || !out->lms || !out->match_idx || !out->match_dist || !out->n_matches)
        return "bad argument";
    return hs_first({ hs_kf_votes_why(T, 1, w.q_off, out->weights, out->max_slot, out->max_count, nullptr, nullptr, 0, w.n_ordered),
                      hs_local_keyframes_why(T->n_kf, out->weights, T->kf_bad, d_neigh, neigh_cap, d_parent, out->local, out->n_local),
                      hs_local_points_why(T, out->local, d_frame_lm, n_assoc, out->frame_remove, out->sel, cap, out->n_sel, w.points.base),
                      hs_landmark_gather_why(d_lms, T->L, out->sel, out->n_sel, cap, out->lms),
                      hs_search_by_projection_why(F, out->lms, cap, pp, out->match_idx, out->match_dist, out->n_matches) });
}
int hs_local_map_search_enqueue(hs_orb* h, const hs_kf_table* T, const int32_t* d_frame_lm, int n_assoc, const int32_t* d_neigh, int neigh_cap, const int32_t* d_parent,
                                int n_max_local_keyframes, int n_neighbor_keyframes, const hs_frame_view* F, const hs_pose_view* d_pose, const hs_landmark* d_lms,
                                const hs_proj_params* pp, int cap, const hs_local_map_out* out, const HsLocalMapWork& w, hipStream_t s)
{
    hs_launch_local_map_query(n_assoc, w.q_off, s);
    hs_kf_votes_enqueue(T, 1, w.q_off, d_frame_lm, nullptr, 1, 1, out->weights, out->max_slot, out->max_count, nullptr, nullptr, 0, w.n_ordered, s);
    hs_launch_local_keyframes(T->n_kf, out->weights, T->kf_bad, d_neigh, neigh_cap, d_parent, n_max_local_keyframes, n_neighbor_keyframes, out->local, out->n_local, s);
    hs_launch_local_points(*T, out->local, d_frame_lm, n_assoc, out->frame_remove, out->sel, cap, out->n_sel, w.points, s);
    hs_launch_landmark_gather(d_lms, T->L, out->sel, out->n_sel, cap, out->lms, s);
    return hs_search_by_projection_enqueue(h, F, d_pose, out->lms, cap, pp, out->match_idx, out->match_dist, out->n_matches, s);
}

namespace {
// both public forms; refuse: the posed form without a pose
int local_map_search(hs_orb* h, bool refuse, const hs_kf_table* T, const int32_t* d_frame_lm, int n_assoc, const int32_t* d_neigh, int neigh_cap,
                     const int32_t* d_parent, int n_max_local_keyframes, int n_neighbor_keyframes, const hs_frame_view* F, const hs_pose_view* d_pose,
                     const hs_landmark* d_lms, const hs_proj_params* pp, int cap, const hs_local_map_out* out, void* d_work, void* stream)
{
    HsWorkCursor c(d_work);
    const HsLocalMapWork w(c, T ? T->L : 0);
    return hs_device_call(h, refuse ? "bad argument" : hs_local_map_search_why(T, d_frame_lm, n_assoc, d_neigh, neigh_cap, d_parent, F, d_lms, pp, cap, out, w), stream,
                          [&](hipStream_t s) {
        return hs_local_map_search_enqueue(h, T, d_frame_lm, n_assoc, d_neigh, neigh_cap, d_parent, n_max_local_keyframes, n_neighbor_keyframes, F, d_pose, d_lms, pp, cap,
                                           out, w, s);
    });
}
}  // namespace

extern "C" {

size_t hs_local_points_work_bytes(int L) { return HsLocalPointsWork::bytes(L); }
size_t hs_local_map_work_bytes(int L) { return HsLocalMapWork::bytes(L); }

int hs_local_keyframes_device(hs_orb* h, int n_kf, const int32_t* d_weights, const uint8_t* d_kf_bad, const int32_t* d_neigh, int neigh_cap,
                              const int32_t* d_parent, int n_max_local_keyframes, int n_neighbor_keyframes, uint8_t* d_local, int32_t* d_n_local, void* stream)
{
    return hs_device_call(h, hs_local_keyframes_why(n_kf, d_weights, d_kf_bad, d_neigh, neigh_cap, d_parent, d_local, d_n_local), stream, [&](hipStream_t s) {
        hs_launch_local_keyframes(n_kf, d_weights, d_kf_bad, d_neigh, neigh_cap, d_parent, n_max_local_keyframes, n_neighbor_keyframes, d_local, d_n_local, s);
    });
}

int hs_local_keyframes(hs_orb* h, int n_kf, const int32_t* weights, const uint8_t* kf_bad, const int32_t* neigh, int neigh_cap, const int32_t* parent,
                       int n_max_local_keyframes, int n_neighbor_keyframes, uint8_t* local, int32_t* n_local)
{
    if (!h) return HS_ERR_INVALID;
    if (n_kf < 0 || neigh_cap < 0 || !n_local || (n_kf > 0 && (!weights || !kf_bad || !parent || !local || (neigh_cap > 0 && !neigh))))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (n_neighbor_keyframes < 0 || n_neighbor_keyframes > neigh_cap) return hs_fail(h, HS_ERR_INVALID, "n_neighbor_keyframes must be in [0, neigh_cap]");
    if (!hs_index_range_ok(neigh, (size_t)n_kf * neigh_cap, -1, n_kf) || !hs_index_range_ok(parent, (size_t)n_kf, -1, n_kf))
        return hs_fail(h, HS_ERR_INVALID, "a neighbour or parent slot outside [-1, n_kf)");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    HsStage st(h);
    int32_t *d_w, *d_neigh, *d_parent, *d_n;
    uint8_t *d_bad, *d_local;
    st.in(&d_w, (size_t)n_kf, weights); st.in(&d_bad, (size_t)n_kf, kf_bad); st.in(&d_neigh, (size_t)n_kf * neigh_cap, neigh); st.in(&d_parent, (size_t)n_kf, parent);
    st.out(&d_local, (size_t)n_kf, local); st.out(&d_n, 1, n_local);
    const int rc = st.begin();
    if (rc != HS_OK) return rc;
    hs_launch_local_keyframes(n_kf, d_w, d_bad, d_neigh, neigh_cap, d_parent, n_max_local_keyframes, n_neighbor_keyframes, d_local, d_n, st.stream());
    return st.finish();
}

int hs_local_points_device(hs_orb* h, const hs_kf_table* T, const uint8_t* d_local, const int32_t* d_frame_lm, int n_assoc, uint8_t* d_frame_remove,
                           int32_t* d_sel, int cap, int32_t* d_n_sel, void* d_work, void* stream)
{
    return hs_device_call(h, hs_local_points_why(T, d_local, d_frame_lm, n_assoc, d_frame_remove, d_sel, cap, d_n_sel, d_work), stream, [&](hipStream_t s) {
        HsWorkCursor c(d_work);
        hs_launch_local_points(*T, d_local, d_frame_lm, n_assoc, d_frame_remove, d_sel, cap, d_n_sel, HsLocalPointsWork(c, T->L), s);
    });
}

int hs_local_points(hs_orb* h, const hs_kf_table* T, const uint8_t* local, const int32_t* frame_lm, int n_assoc, uint8_t* frame_remove,
                    int32_t* sel, int cap, int32_t* n_sel)
{
    if (!h) return HS_ERR_INVALID;
    if (!T || T->L < 0 || T->n_kf < 0 || n_assoc < 0 || cap < 0 || !n_sel || (cap > 0 && !sel) || (n_assoc > 0 && (!frame_lm || !frame_remove)) ||
        !T->lm_obs_offsets || (T->L > 0 && !T->lm_bad) || (T->n_kf > 0 && !local))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    const int L = T->L, n_kf = T->n_kf;
    if (!hs_csr_ok(T->lm_obs_offsets, L)) return hs_fail(h, HS_ERR_INVALID, "offsets must be non-negative and non-decreasing");
    const size_t n_obs = (size_t)T->lm_obs_offsets[L];
    if (n_obs > 0 && !T->lm_obs_kf) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (!hs_index_range_ok(T->lm_obs_kf, n_obs, 0, n_kf) || !hs_index_range_ok(frame_lm, (size_t)n_assoc, -1, L))
        return hs_fail(h, HS_ERR_INVALID, "a key-frame slot or landmark index outside the table");
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    HsStage st(h);
    hs_kf_table D = *T;
    int64_t* d_off; int32_t *d_kf, *d_flm, *d_sel, *d_n; uint8_t *d_bad, *d_local, *d_rem, *d_work;
    st.in(&d_off, (size_t)L + 1, T->lm_obs_offsets); st.in(&d_kf, n_obs, T->lm_obs_kf); st.in(&d_bad, (size_t)L, T->lm_bad);
    st.in(&d_local, (size_t)n_kf, local); st.in(&d_flm, (size_t)n_assoc, frame_lm);
    st.out(&d_rem, (size_t)n_assoc, frame_remove); st.out(&d_sel, (size_t)cap, sel); st.out(&d_n, 1, n_sel);
    st.temp(&d_work, hs_local_points_work_bytes(L));
    const int rc = st.begin();
    if (rc != HS_OK) return rc;
    D.lm_obs_offsets = d_off; D.lm_obs_kf = d_kf; D.lm_bad = d_bad;
    D.lm_obs_octave = nullptr; D.lm_nobs = nullptr; D.kf_bad = nullptr; D.kf_id = nullptr;
    HsWorkCursor c(d_work);
    hs_launch_local_points(D, d_local, d_flm, n_assoc, d_rem, d_sel, cap, d_n, HsLocalPointsWork(c, L), st.stream());
    return st.finish();
}

int hs_landmark_gather_device(hs_orb* h, const hs_landmark* d_lms, int L, const int32_t* d_sel, const int32_t* d_n_sel, int cap, hs_landmark* d_out, void* stream)
{
    return hs_device_call(h, hs_landmark_gather_why(d_lms, L, d_sel, d_n_sel, cap, d_out), stream,
                          [&](hipStream_t s) { hs_launch_landmark_gather(d_lms, L, d_sel, d_n_sel, cap, d_out, s); });
}

int hs_local_map_search_device(hs_orb* h, const hs_kf_table* T, const int32_t* d_frame_lm, int n_assoc, const int32_t* d_neigh, int neigh_cap,
                               const int32_t* d_parent, int n_max_local_keyframes, int n_neighbor_keyframes, const hs_frame_view* F,
                               const hs_landmark* d_lms, const hs_proj_params* pp, int cap, const hs_local_map_out* out, void* d_work, void* stream)
{
    return local_map_search(h, false, T, d_frame_lm, n_assoc, d_neigh, neigh_cap, d_parent, n_max_local_keyframes, n_neighbor_keyframes, F, nullptr, d_lms, pp, cap, out,
                            d_work, stream);
}
// the search reads the pose from device memory (hs_search_by_projection_posed_device)
int hs_local_map_search_posed_device(hs_orb* h, const hs_kf_table* T, const int32_t* d_frame_lm, int n_assoc, const int32_t* d_neigh, int neigh_cap,
                                     const int32_t* d_parent, int n_max_local_keyframes, int n_neighbor_keyframes, const hs_frame_view* F,
                                     const hs_pose_view* d_pose, const hs_landmark* d_lms, const hs_proj_params* pp, int cap, const hs_local_map_out* out,
                                     void* d_work, void* stream)
{
    return local_map_search(h, !d_pose, T, d_frame_lm, n_assoc, d_neigh, neigh_cap, d_parent, n_max_local_keyframes, n_neighbor_keyframes, F, d_pose, d_lms, pp, cap, out,
                            d_work, stream);
}

}  // extern "C"
