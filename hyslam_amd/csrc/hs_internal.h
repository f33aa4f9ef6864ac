// hs_internal.h — shared declarations of the HIP implementation behind include/hyslam_amd.h.
// gfx950 (MI355X) only: wave64, 160 KiB LDS/CU.  Compiled with -ffp-contract=off: several results
// (resize tables, fastAtan2, rBRIEF rotation) are defined by separately rounded fp32 operations.
#pragma once
#include <algorithm>
#include <atomic>
#include <string>
#include <type_traits>
#include <vector>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/hyslam_amd.h"
#include "hs_work.h"                // the caller-owned work areas (d_work) and hs_up256

#define HS_MAX_LEVELS 16
#define HS_EDGE 19                 // EDGE_THRESHOLD, ORBExtractor.cpp:74
#define HS_BORDER 16               // minBorderX = EDGE_THRESHOLD-3, ORBExtractor.cpp:413
#define HS_MAX_CELL_H 125           // tallest FAST cell (the FAST kernel's LDS tile holds hcell + 6 rows; list entries keep the row in 7 bits)
#define HS_QT_MAX_NODES 2048       // quadtree list capacity in LDS of the general instance (>= largest per-level quota + 8)
#define HS_QT_LARGE_NODES 3328     // ... of the large-list instance (rectangles in global scratch, no points in LDS: 161.9 KB of the CU's 160 KiB); quotas up to 3320 per level
#define HS_QT_THREADS 1024

// Per-level geometry and buffers; lives in device memory, read through scalar loads.
struct HsLevel {
    int32_t w, h;                  // level size (ORBExtractor.cpp:568-569)
    int32_t pitch;                 // row pitch of the level buffer (levels >= 1)
    int32_t _r0;
    uint64_t img_stride;           // bytes between consecutive images of this level's buffer
    uint8_t* base;                 // level buffer (levels >= 1; level 0 is the caller's image)
    // FAST cell grid (ORBExtractor.cpp:413-428)
    int32_t ncols, nrows, wcell, hcell;
    int32_t cell_begin;            // first block index of this level in the all-levels cell launch
    // FAST work items (kernels_fast.hip): one item = `grp_cells` horizontally adjacent cells of one cell row
    int32_t grp_cells, ngroups;    // cells per item (the last item of a row may hold fewer), items per cell row
    int32_t item_begin;            // first item of this level within one image's item list
    int32_t inv_wcell, inv_wcell1; // ceil(65536 / wcell), ceil(65536 / (wcell + 1)): x / wcell == (x * inv) >> 16 for x < 256
    // DistributeOctTree inputs (ORBExtractor.cpp:179-203,475-476)
    int32_t qt_w, qt_h;            // maxBorderX-minBorderX, maxBorderY-minBorderY
    int32_t n_ini;                 // round(qt_w / qt_h)
    float   hx;                    // qt_w / n_ini
    int32_t quota;                 // mnFeaturesPerLevel[level]
    // geometric-key tables of the count-domain quadtree (kernels_quadtree.hip), built on the host from the level geometry: cell index of every
    // pixel column within its root / of every pixel row at the depth of the histogram pyramid, first column of roots 1..7; nullptr = none
    const uint8_t* qt_xtab;        // [qt_w + 1], 16-byte aligned, padded to a multiple of 16
    const uint8_t* qt_ytab;        // [qt_h + 1]
    int32_t qt_rbound[8];
    // round 4: the FAST kernel computes every candidate's geometric key itself and leaves, per (image, level), the HISTOGRAM of the keys (u16
    // counters packed in u32) and the BEST candidate of every deepest cell (u64 keys) in global memory: the quadtree kernel starts from them
    // instead of gathering the candidates.  Offsets of this level inside one image's arrays (entries); 0xFFFFFFFF = the level has no tables.
    uint32_t qt_hist_off;          // in u32 (= 2 cells)
    uint32_t qt_best_off;          // in u64 (= 1 cell)
    // candidate / selection storage (entries, per image)
    int32_t cand_cap;
    int32_t sel_cap;
    uint64_t cand_off;             // offset of this level inside one image's candidate arrays
    int32_t sel_off;               // offset inside one image's selection arrays
    // resize tables (cv::resize INTER_LINEAR, fixed point), device pointers; level >= 1
    int32_t xmax;
    const int16_t* xofs;           // [w]
    const int16_t* ialpha;         // [w][2]
    const int16_t* yofs;           // [h]
    const int16_t* ibeta;          // [h][2]
    float scale;                   // mvScaleFactor[level]
    float kp_size;                 // (int)(31*scale)
    // two-levels-per-launch pyramid kernel (kernels_pyramid.hip): this level and the next one are produced by one workgroup per tile of the NEXT
    // level; 0 = this pair is not fused.  Tile width of the next level, LDS rows for this level's region / the source rectangle, source pitch.
    int32_t fuse_tbx, fuse_ar, fuse_sr, fuse_pitch;
    int32_t chain_n;               // levels produced by a k_resize_chain launch that starts at this level (0: none)
    int32_t _r1;
};

struct HsImg0 {                    // level 0 = the caller's frames; images [0,split) from base, the rest from base2
    const uint8_t* base;           // (left / right frames of a stereo batch go through one launch sequence)
    const uint8_t* base2;
    int32_t split;
    uint64_t row_stride;
    uint64_t img_stride;
};
__host__ __device__ inline const uint8_t* hs_img0_ptr(const HsImg0& I, int img)
{
    return img < I.split ? I.base + (size_t)img * I.img_stride : I.base2 + (size_t)(img - I.split) * I.img_stride;
}

// Pointers that reach a kernel through a struct in memory (HsLevel::base, the tables) have no provable address space and compile to
// FLAT loads, which count on lgkmcnt as well as vmcnt: every LDS wait then also waits for them.  These helpers assert "global".
#define HS_GLOBAL __attribute__((address_space(1)))
typedef uint32_t hs_u32x4 __attribute__((ext_vector_type(4)));
template <typename T> __device__ __forceinline__ T hs_gload(const void* p) { return *(const HS_GLOBAL T*)(uintptr_t)p; }
// read-only tables at a wave-uniform address: the constant address space lets the compiler use scalar loads (SGPR result, no VALU/VMEM slot)
#define HS_CONSTANT __attribute__((address_space(4)))
template <typename T> __device__ __forceinline__ T hs_cload(const void* p) { return *(const HS_CONSTANT T*)(uintptr_t)p; }
// element `idx` of a read-only int16 table (4-byte aligned base) at a wave-uniform index: there are no sub-dword scalar loads, so the
// containing dword is fetched and the half picked with SALU (a plain int16 load would be a VECTOR load and put the value in a VGPR)
__device__ __forceinline__ int hs_cload_i16(const int16_t* base, int idx)
{
    const uint32_t w = hs_cload<uint32_t>(reinterpret_cast<const uint8_t*>(base) + 4 * (size_t)(idx >> 1));
    return (int)(int16_t)((idx & 1) ? (w >> 16) : (w & 0xFFFFu));
}
// a pointer the compiler must keep in SGPRs (so that `uniform base + 32-bit lane offset` becomes the saddr form of global_load)
__device__ __forceinline__ const uint8_t* hs_uniform_ptr(const uint8_t* p)
{
    const uint64_t v = (uint64_t)(uintptr_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (const uint8_t*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}
template <typename T> __device__ __forceinline__ T hs_gload_off(const uint8_t* uniform_base, uint32_t lane_off)
{
    return *(const HS_GLOBAL T*)((const HS_GLOBAL uint8_t*)(uintptr_t)uniform_base + lane_off);
}
template <typename T> __device__ __forceinline__ void hs_gstore(void* p, T v) { *(HS_GLOBAL T*)(uintptr_t)p = v; }
// inclusive prefix sum over the 64 lanes of a wave (DPP row shifts + row broadcasts: six VALU adds, no LDS)
__device__ __forceinline__ int wave_scan_incl(int x)
{
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true);      // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true);      // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true);      // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true);      // row_shr:8   -> inclusive within each row of 16
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);     // row_bcast:15 into rows 1 and 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);     // row_bcast:31 into rows 2 and 3
    return x;
}

struct HsOut {                     // extractor outputs, split the same way
    hs_keypoint* kps; uint8_t* desc; int32_t* n;
    hs_keypoint* kps2; uint8_t* desc2; int32_t* n2;
    int32_t split;
    int32_t cap;
};

#include "hs_pyramid.h"             // the image pyramid: its records, limits, planners' interface and launch function
#include "hs_fast.h"                // the FAST stage: its records, limits, work-unit schedule, planner's interface and launch function

#define HS_STRIP_ENTRY_BYTES 16
#define HS_STRIP_SHIFT 5           // right keypoints are binned into strips of 32 rows (kernels_stereo.hip)
// A strip entry carries everything the candidate test needs, so that the matcher's chain of dependent loads is entry -> descriptor instead of
// index -> keypoint record -> descriptor: the right keypoint's u, its octave, its index and its row band CUT TO THE STRIP (two 5-bit row numbers:
// a left keypoint that scans strip s has its row in [32 s, 32 s + 31], so the cut band decides exactly what the whole band decides).
struct __attribute__((aligned(16))) HsStripEntry { float uR; int32_t octave; uint32_t idx_band; uint32_t _pad; };   // idx_band = iR | lo << 16 | hi << 24
static_assert(sizeof(HsStripEntry) == HS_STRIP_ENTRY_BYTES, "hs_api.hip sizes the strip lists with HS_STRIP_ENTRY_BYTES");
#define HS_STRIPS_MAX 2048         // 65536 rows / 32
// The stereo front end (extract L + R, then match; hs_stereo_frontend_batch_device): the describe launch carries one extra workgroup per RIGHT
// image that bins the image's selected keypoints into the strips (position, level and list index are known since the quadtree kernel; the
// describe workgroups next to it fill in angle and descriptor) — no k_stereo_strips launch.  enabled = 0: a plain describe launch.
struct HsStripFuse { int32_t enabled, n_rows, n_strips, _r; float size_ref; int32_t* strip_count; HsStripEntry* strip_list; };
inline int hs_stereo_strips(int n_rows) { return (n_rows > 0 ? ((n_rows - 1) >> 5) : 0) + 1; }

// kernels_*.hip launchers (all asynchronous on `s`)
void hs_launch_quadtree(const HsLevel* d_lv, int nlevels, int batch, int total_cells,
                        const uint2* cand, const int32_t* cell_count, uint64_t cand_img_stride,
                        uint32_t* pts_xy, uint32_t* pts_sk, uint16_t* pt_node, int32_t* cand_count,
                        uint32_t* sel_xys, int32_t* sel_count, int sel_img_stride, uint16_t* sel_perm /*spatial order per (image, level)*/, int force_point_domain, int level_first, int level_count,
                        uint32_t* qhist /*nullptr: the FAST launch left no keys — gather*/, unsigned long long* qbest, uint32_t qhist_img_stride, uint32_t qbest_img_stride,
                        int keep_points /*debug: gather the candidates into pts_* even when the keys make it unnecessary*/,
                        int list_mode /*0: the general instance; 1: every level's quota + 8 <= hs_quadtree_small_nodes(), launches of > 256 workgroups may use the two-per-CU instance;
                                        2: a quota + 8 > HS_QT_MAX_NODES: the large-list instance (needs rect_scratch)*/,
                        uint8_t* rect_scratch /*list_mode 2: batch * nlevels * hs_quadtree_large_scratch_bytes(), indexed by (image, level)*/, hipStream_t s);
// kernels_preprocess.hip: ImageProcessing::PreProcessImg (camera scale + grey) between the upload and the pyramid
void hs_preprocess_out_size(int w, int h, float fscale, int* ow, int* oh);
int  hs_preprocess_mode(int w, int h, int ow, int oh, float fscale);      // 0 copy, 1 the 2x2 area path (scale exactly 0.5), 2 bilinear
void hs_launch_preprocess(const uint8_t* d_src, int sw, int sh, size_t src_row_stride, size_t src_img_stride, int channels, int rgb, float fscale,
                          uint8_t* d_dst, int dw, int dh, size_t dst_row_stride, size_t dst_img_stride, int dst_may_pad /*rows may be written up to the next multiple of 4 columns*/,
                          int batch, hipStream_t s);
int hs_quadtree_small_nodes();
size_t hs_quadtree_large_scratch_bytes();
void hs_launch_describe(const HsLevel* d_lv, int nlevels, HsImg0 img0, int batch,
                        const uint32_t* sel_xys, const int32_t* sel_count, const uint16_t* sel_perm, int sel_img_stride, int max_sel,
                        const uint16_t* taps7, HsOut out, hipStream_t s, bool fast_taps, HsStripFuse strips);
void hs_launch_stereo(const hs_keypoint* kpsL, const uint8_t* descL, const int32_t* nL,
                      const hs_keypoint* kpsR, const uint8_t* descR, const int32_t* nR,
                      int pairs, int cap, hs_stereo_params sp, float* uRight, float* depth,
                      int32_t* best_dist /*[pairs][cap] scratch*/,
                      int32_t* strip_count /*[pairs][strips]*/, void* strip_list /*[pairs][strips][cap] entries of HS_STRIP_ENTRY_BYTES*/, hipStream_t s);
void hs_launch_stereo_median(const int32_t* nL, int pairs, int cap, float* uRight, float* depth, const int32_t* best_dist, float th_high,
                             int32_t* strip_count /*zero on entry of hs_launch_stereo; zeroed again here*/, int n_rows, hipStream_t s);
// the matcher alone, on strips that the describe launch of the stereo front end has already binned (HsStripFuse)
void hs_launch_stereo_match_only(const hs_keypoint* kpsL, const uint8_t* descL, const int32_t* nL,
                                 const hs_keypoint* kpsR, const uint8_t* descR, const int32_t* nR,
                                 int pairs, int cap, hs_stereo_params sp, float* uRight, float* depth, int32_t* best_dist,
                                 const int32_t* strip_count, const void* strip_list, hipStream_t s);

// kernels_match.hip
size_t hs_frame_grid_bytes(int n);               // cells + cell lists of n keypoints
void hs_launch_frame_grid(const hs_frame_view& F, const hs_keypoint* d_kps, int8_t* d_cell /*hs_frame_grid_bytes(n)*/, bool with_lists, hipStream_t s);
void hs_launch_search_projection(const hs_frame_view& F, const hs_keypoint* d_kps, const uint8_t* d_desc, const float* d_uR,
                                 const int32_t* d_obs, const int8_t* d_cell, const hs_landmark* d_lms, int L, const hs_proj_params& pp,
                                 int32_t* d_match_idx, float* d_match_dist, int32_t* d_winner, float* d_prev_angle_scratch,
                                 int32_t* d_n_matches, hipStream_t s, const hs_pose_view* d_pose = nullptr /*device: read the pose from it, not from F*/);
void hs_launch_bow(const int32_t* d_pair_a, const int32_t* d_pair_b, int n_pairs,
                   const int32_t* d_ptr1, const int32_t* d_idx1, const int32_t* d_ptr2, const int32_t* d_idx2,
                   const uint8_t* d_desc1, const uint8_t* d_desc2, const uint8_t* d_keep1, const uint8_t* d_keep2,
                   const float* F12, float size_ref, float sigma_ref, float thr, float ratio,
                   int32_t* d_match12, int n1, const hs_keypoint* d_kps1, const hs_keypoint* d_kps2, float* d_angle2_scratch,
                   int check_rotation, int32_t* d_self_scratch, int32_t* d_n_matches, hipStream_t s);
void hs_launch_knn2(const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int32_t* d_bi, int32_t* d_bd, int32_t* d_sd, hipStream_t s);
void hs_launch_sim3_projection(const hs_frame_view& F, const hs_keypoint* d_kps, const uint8_t* d_desc, const int8_t* d_cell,
                               const float* R9, const float* t3, const float* Ow3, const hs_landmark* d_lms, int L, float th, float th_low,
                               float* d_geo, uint8_t* d_kp_matched, int32_t* d_match_idx, int32_t* d_n_matches, hipStream_t s);
void hs_launch_sim3_search(const hs_frame_view& F1, const hs_keypoint* d_kps1, const uint8_t* d_desc1, const int8_t* d_cell1,
                           const hs_frame_view& F2, const hs_keypoint* d_kps2, const uint8_t* d_desc2, const int8_t* d_cell2,
                           const hs_landmark* d_lms1, const hs_landmark* d_lms2, const float* sR21, const float* t21, const float* sR12, const float* t12,
                           float th, float th_high, int32_t* d_m1, int32_t* d_m2, int32_t* d_match12, int32_t* d_n_found, hipStream_t s);
void hs_launch_knn2_records(const uint8_t* d_recs, size_t stride, int world, int rank, int cap, size_t off_desc,
                            int32_t* d_bi, int32_t* d_bd, int32_t* d_sd, hipStream_t s);
void hs_launch_stream_copy(void* d_dst, const void* d_src, size_t bytes, int width, hipStream_t s);
void hs_launch_bow_legacy(const int32_t* d_pair_a, const int32_t* d_pair_b, int n_pairs,
                          const int32_t* d_ptr1, const int32_t* d_idx1, const int32_t* d_ptr2, const int32_t* d_idx2,
                          const uint8_t* d_desc1, const uint8_t* d_desc2, const uint8_t* d_keep1, const uint8_t* d_keep2, float thr, float ratio,
                          int32_t* d_match12, int n1, int n2, const hs_keypoint* d_kps1, const hs_keypoint* d_kps2, float* d_angle1_scratch,
                          int check_orientation, int32_t* d_self_scratch, uint32_t* d_taken2, int32_t* d_n_matches, hipStream_t s);
void hs_launch_bow_transform(int n, const uint8_t* d_desc, const int32_t* d_cb, const int32_t* d_cc, const uint8_t* d_ndesc, const int32_t* d_word,
                             const float* d_weight, int levels, int levelsup, int32_t* d_out_word, float* d_out_weight, int32_t* d_out_node, hipStream_t s);
void hs_launch_search_init(const hs_frame_view& F2, const hs_keypoint* d_kps2, const uint8_t* d_desc2, const int8_t* d_cell2,
                           const hs_keypoint* d_kps1, const uint8_t* d_desc1, int n1, const float* d_prev_xy, float window, float th_low, float nnratio,
                           int32_t* d_owner, int32_t* d_odist, float* d_angle_scratch, int32_t* d_self_scratch, int32_t* d_n_matches, hipStream_t s);

// ---- the local map (kernels_localmap.hip; entry points in hs_localmap.hip)
void hs_launch_local_keyframes(int n_kf, const int32_t* d_weights, const uint8_t* d_kf_bad, const int32_t* d_neigh, int neigh_cap, const int32_t* d_parent,
                               int n_max, int n_neighbor, uint8_t* d_local, int32_t* d_n_local, hipStream_t s);
void hs_launch_local_points(const hs_kf_table& T, const uint8_t* d_local, const int32_t* d_frame_lm, int n_assoc, uint8_t* d_frame_remove,
                            int32_t* d_sel, int cap, int32_t* d_n_sel, const HsLocalPointsWork& w, hipStream_t s);
void hs_launch_landmark_gather(const hs_landmark* d_lms, int L, const int32_t* d_sel, const int32_t* d_n_sel, int cap, hs_landmark* d_out, hipStream_t s);
void hs_launch_local_map_query(int n_assoc, int64_t* d_q_off, hipStream_t s);

// ---- host entry points that work on a handle (hs_api.hip, kernels_landmark.hip, kernels_bow.hip, kernels_place.hip, hs_kfgraph.hip, hs_localmap.hip, hs_comm.hip) ----
// hs_orb is opaque outside hs_api.hip; the other translation units reach it through these four accessors (defined in hs_api.hip).
void hs_set_error(hs_orb* h, const char* msg);
int hs_orb_device_of(const hs_orb* h);
hipStream_t hs_orb_stream_of(const hs_orb* h);
// claims `bytes` of the handle's grow-only device scratch arena and invalidates what an earlier claim handed out; a regrow synchronises the
// handle's stream first, and `user` (the stream the claiming stage enqueues on) where that is another one: earlier work of either may still use
// the block a regrow frees.  No regrow: no wait.  nullptr on failure, the error text set (HS_ERR_HIP)
uint8_t* hs_orb_scratch_of(hs_orb* h, size_t bytes, hipStream_t user);
// the stream a device entry point enqueues on: the caller's, or the handle's where the caller passes NULL
inline hipStream_t hs_stream_or(const hs_orb* h, void* stream) { return stream ? (hipStream_t)stream : hs_orb_stream_of(h); }

inline int hs_fail(hs_orb* h, int code, const std::string& msg) { hs_set_error(h, msg.c_str()); return code; }
// a failed HIP call leaves its code in the runtime's sticky "last error": it is cleared here so that the next successful call sequence on this
// thread does not report it again through hipGetLastError()
#define HIP_TRY(h, expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { (void)hipGetLastError(); \
    return hs_fail(h, HS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); } } while (0)

// The public form of every enqueue-only `_device` entry point of the resident chain.  `why` is the entry point's predicate over its
// arguments — pure host code, the refusal's text or nullptr — and `enqueue(stream)` its launches with no check in them: a composite's predicate is
// its stages' predicates and its enqueue their enqueues, so this is the one place a chain sets the device and asks for the last error, once each,
// and a refused call enqueues, copies and allocates nothing.  enqueue returns void, or an HS_ status where it makes a HIP call that is no launch.
inline const char* hs_bad(bool refused) { return refused ? "bad argument" : nullptr; }
template <class Enqueue> int hs_device_call(hs_orb* h, const char* why, void* stream, Enqueue enqueue)
{
    if (!h) return HS_ERR_INVALID;
    if (why) return hs_fail(h, HS_ERR_INVALID, why);
    HIP_TRY(h, hipSetDevice(hs_orb_device_of(h)));
    if constexpr (std::is_void<decltype(enqueue(hipStream_t()))>::value) enqueue(hs_stream_or(h, stream));
    else { const int rc = enqueue(hs_stream_or(h, stream)); if (rc != HS_OK) return rc; }
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

// argument checks of the host forms over an observation table (hs_kfgraph.hip, hs_localmap.hip): a CSR of `n` rows has offsets[0] >= 0 and is
// non-decreasing; every index lies in [lo, limit)
inline bool hs_csr_ok(const int64_t* off, int n)
{
    if (off[0] < 0) return false;
    for (int i = 0; i < n; i++) if (off[i + 1] < off[i]) return false;
    return true;
}
inline bool hs_index_range_ok(const int32_t* v, size_t n, int lo, int limit)
{
    for (size_t i = 0; i < n; i++) if (v[i] < lo || v[i] >= limit) return false;
    return true;
}

#define HS_STAGE_MAX_PIECES 17      // the largest user: bow_host (hs_api.hip)
// bytes claimed past the last piece.  No kernel needs them: under hs_debug_poison every host-pointer entry point was run with the arena filled
// and the gaps checked (tests/test_gpu_poison.py) — no piece was written past its registered size, nothing wrote into the slack,
// and every result was independent of the fill, so nothing reads it either.  It is kept as the guard band that check watches: a store past the
// last piece lands here, inside the arena, and is reported instead of reaching whatever follows the allocation.
#define HS_STAGE_SLACK 4096

// ---- workspace poisoning (hs_debug_poison, include/hyslam_amd.h).  g_hs_poison is -1 (off) or the byte.  With it off the whole
// cost is one relaxed load per HsStage::begin() and per device allocation: no launch, copy or synchronisation is added anywhere.
extern std::atomic<int> g_hs_poison;                              // hs_api.hip
inline int hs_poison_byte() { return g_hs_poison.load(std::memory_order_relaxed); }
hipError_t hs_poison_fill(void* p, size_t bytes, int byte);      // hs_api.hip: hipMemset, then waits for it
// every device allocation of the library passes through here right after its hipMalloc
inline hipError_t hs_poison_fresh(void* p, size_t bytes) { const int b = hs_poison_byte(); return b < 0 || !p || !bytes ? hipSuccess : hs_poison_fill(p, bytes, b); }
struct HsPoisonGaps { int32_t n, _r; unsigned long long begin[HS_STAGE_MAX_PIECES], end[HS_STAGE_MAX_PIECES]; };   // arena offsets; gap i follows piece i
#define HS_POISON_REPORT_BYTES 256  // behind the slack while poisoning is on: one u64 per gap, the offset of its first changed byte (all ones: none)
void hs_launch_poison_check(const uint8_t* d_base, const HsPoisonGaps& gaps, int byte, unsigned long long* d_first, hipStream_t s);   // hs_api.hip
void hs_poison_violation();                                       // bumps what hs_debug_poison_violations() returns

// The device side of one host-pointer call, laid out in the handle's scratch arena.  The caller registers every piece (element type, count and
// what to copy; add() below is the only place a size is added up), begin() claims the arena for their sum, hands every piece its 256-byte
// aligned address (distinct and valid also for a count of 0) and enqueues the uploads in registration order; after the launches finish() checks them, enqueues
// the downloads in registration order and synchronises.  No heap allocation; one call at a time per handle (begin() invalidates the last layout).
// Under hs_debug_poison begin() first fills the whole claim [0, total + HS_STAGE_SLACK) with the byte, on the call's stream, and finish() checks on
// the device, behind the launches, that every gap between two pieces and the slack still hold it (HS_ERR_POISON; the downloads are made all the same).
class HsStage {
public:
    explicit HsStage(hs_orb* h) : h_(h), s_(hs_orb_stream_of(h)) {}
    HsStage(hs_orb* h, hipStream_t s) : h_(h), s_(s) {}           // a device form that runs on the caller's stream: temporaries only
    hipStream_t stream() const { return s_; }
    template <class T> void temp(T** d, size_t count) { add(d, count * sizeof(T), nullptr, nullptr, 0); }
    // src == nullptr (an optional input that is absent): the piece is laid out, nothing is copied
    template <class T> void in(T** d, size_t count, const T* src) { add(d, count * sizeof(T), src, nullptr, 0); }
    // the first `n_back` of `count` elements come back to dst (default: all of them)
    template <class T> void out(T** d, size_t count, T* dst, size_t n_back = SIZE_MAX) { add(d, count * sizeof(T), nullptr, dst, std::min(n_back, count) * sizeof(T)); }
    template <class T> void inout(T** d, size_t count, T* host) { add(d, count * sizeof(T), host, host, count * sizeof(T)); }
    int begin()
    {
        if (n_ > HS_STAGE_MAX_PIECES) return hs_fail(h_, HS_ERR_INVALID, "internal: a host call stages more than HS_STAGE_MAX_PIECES pieces");
        poison_ = hs_poison_byte();
        const size_t claim = total_ + HS_STAGE_SLACK;
        uint8_t* base = hs_orb_scratch_of(h_, claim + (poison_ >= 0 ? HS_POISON_REPORT_BYTES : 0), s_);
        if (!base) return HS_ERR_HIP;
        if (poison_ >= 0) {
            base_ = base;
            HIP_TRY(h_, hipMemsetAsync(base, poison_, claim, s_));
            HIP_TRY(h_, hipMemsetAsync(base + claim, 0xFF, HS_POISON_REPORT_BYTES, s_));
        }
        for (int i = 0; i < n_; i++) {
            const Piece& p = p_[i];
            *p.dev = base + p.off;
            if (p.src && p.bytes) HIP_TRY(h_, hipMemcpyAsync(*p.dev, p.src, p.bytes, hipMemcpyHostToDevice, s_));
        }
        return HS_OK;
    }
    int finish()
    {
        HIP_TRY(h_, hipGetLastError());
        unsigned long long first[HS_STAGE_MAX_PIECES];
        if (poison_ >= 0) { const int rc = check_enqueue(first); if (rc != HS_OK) return rc; }
        for (int i = 0; i < n_; i++)
            if (p_[i].back) HIP_TRY(h_, hipMemcpyAsync(p_[i].dst, *p_[i].dev, p_[i].back, hipMemcpyDeviceToHost, s_));
        HIP_TRY(h_, hipStreamSynchronize(s_));
        return poison_ >= 0 ? check_report(first) : HS_OK;
    }
    // for a call that brings its results back by itself (hs_bow_vector): the poison check alone, synchronous; HS_OK while poisoning is off
    int verify()
    {
        if (poison_ < 0) return HS_OK;
        unsigned long long first[HS_STAGE_MAX_PIECES];
        const int rc = check_enqueue(first);
        if (rc != HS_OK) return rc;
        HIP_TRY(h_, hipStreamSynchronize(s_));
        return check_report(first);
    }
private:
    struct Piece { void** dev; size_t off, bytes, back; const void* src; void* dst; };
    template <class T> void add(T** d, size_t bytes, const void* src, void* dst, size_t back)
    {
        if (n_ < HS_STAGE_MAX_PIECES) { p_[n_] = Piece{ reinterpret_cast<void**>(d), total_, bytes, back, src, dst }; total_ += hs_up256(std::max<size_t>(bytes, 1)); }
        n_++;                       // past the capacity: begin() refuses
    }
    int check_enqueue(unsigned long long* first)
    {
        if (n_ == 0) return HS_OK;
        HsPoisonGaps g{};
        g.n = n_;
        for (int i = 0; i < n_; i++) { g.begin[i] = p_[i].off + p_[i].bytes; g.end[i] = i + 1 < n_ ? p_[i + 1].off : total_ + HS_STAGE_SLACK; }
        unsigned long long* d_first = reinterpret_cast<unsigned long long*>(base_ + total_ + HS_STAGE_SLACK);
        hs_launch_poison_check(base_, g, poison_, d_first, s_);
        HIP_TRY(h_, hipGetLastError());
        HIP_TRY(h_, hipMemcpyAsync(first, d_first, (size_t)n_ * sizeof(unsigned long long), hipMemcpyDeviceToHost, s_));
        return HS_OK;
    }
    int check_report(const unsigned long long* first)
    {
        for (int i = 0; i < n_; i++) {
            if (first[i] == ~0ull) continue;
            hs_poison_violation();
            const bool slack = i + 1 == n_ && first[i] >= total_;
            return hs_fail(h_, HS_ERR_POISON, "workspace poison: piece " + std::to_string(i) + " (arena offset " + std::to_string(p_[i].off) + ", " + std::to_string(p_[i].bytes) +
                           " bytes) was written past its end: first changed byte at arena offset " + std::to_string(first[i]) + (slack ? " (in the slack)" : " (in its padding)"));
        }
        return HS_OK;
    }
    hs_orb* h_; hipStream_t s_; int n_ = 0; size_t total_ = 0; Piece p_[HS_STAGE_MAX_PIECES];
    int poison_ = -1; uint8_t* base_ = nullptr;
};
