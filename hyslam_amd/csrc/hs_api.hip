// hs_api.hip — host side of the C ABI declared in include/hyslam_amd.h.
// Owns the per-handle device workspace (sized for 288 GB HBM: worst-case candidate storage, no overflow
// paths), the host-computed tables (scale factors, per-level quotas, resize coefficients) and the launch
// sequence.  The whole extraction of a batch is GPU-resident: pyramid -> FAST/NMS cells -> quadtree
// distribution -> blur+orientation+rBRIEF, 10 kernel launches for an 8-level pyramid regardless of batch size.
#include "hs_plan.h"
#include "hs_stereo.h"
#include "hs_track.h"               // hs_search_by_projection_why / _enqueue: the search is a stage of the track chains
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#define HS_VERSION "hyslam_amd 0.1 (gfx950)"

// One owned allocation — device memory, or page-locked host memory with Pinned — and its capacity in elements of T.  Grow-only; it never
// synchronises by itself: whoever regrows a buffer that enqueued work may still use passes the stream to drain (or waits for its own event) first.
// The rule: a regrow waits for EVERY stream that work using the old block may have been enqueued on.  grow(count, drain) waits for one; a buffer
// used from two (the scratch arena: the handle's stream and the stream of a device-form stage) has the second drained by its owner before the
// call (hs_orb_scratch_of).  Nothing relies on hipFree waiting for the device.  Without a regrow neither form waits, launches or copies.
template <class T, bool Pinned = false> struct HsBuf {
    T* p = nullptr; size_t cap = 0;
    HsBuf() = default;
    HsBuf(const HsBuf&) = delete; HsBuf& operator=(const HsBuf&) = delete;
    HsBuf(HsBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    HsBuf& operator=(HsBuf&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~HsBuf() { release(); }
    void release() { if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
    // room for `count` elements; the contents do not survive a regrow, and a failed one leaves the buffer empty
    hipError_t grow(size_t count)
    {
        if (count <= cap) return hipSuccess;
        release();
        const hipError_t e = Pinned ? hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault) : hipMalloc((void**)&p, count * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = count;
        return Pinned ? hipSuccess : hs_poison_fresh(p, count * sizeof(T));      // hs_debug_poison: filled before first use
    }
    hipError_t grow(size_t count, hipStream_t drain)          // ... after everything enqueued on `drain` has finished (a second stream: the rule above)
    {
        if (count <= cap) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(drain);
        return e != hipSuccess ? e : grow(count);
    }
    operator T*() const { return p; }
};
template <class T> using HsPinned = HsBuf<T, true>;

// level-0 frames of a host-pointer call in HBM (d_in), and the camera's frames as uploaded, before PreProcessImg on the device (d_raw)
struct HsFrameStaging { HsBuf<uint8_t> d_in, d_raw; };
// uRight / depth / best distance of the stereo matcher: three arrays that grow on one count
struct HsStereoOut {
    HsBuf<float> ur, depth; HsBuf<int32_t> bd;
    hipError_t grow(size_t entries, hipStream_t drain)
    {
        if (entries <= ur.cap && entries <= depth.cap && entries <= bd.cap) return hipSuccess;
        hipError_t e = hipStreamSynchronize(drain);
        if (e == hipSuccess) e = ur.grow(entries);
        if (e == hipSuccess) e = depth.grow(entries);
        if (e == hipSuccess) e = bd.grow(entries);
        return e;
    }
};

struct hs_orb {
    hs_orb_params p;
    int device = 0;
    // communicators created on this handle (hs_comm_create) BORROW it — its device and its stream: while one is alive hs_orb_destroy only drops
    // the owner's reference and the last hs_comm_destroy frees the handle, so the two destroy calls are safe in either order and on two threads
    std::atomic<bool> owned{true};            // hs_orb_destroy has not been called yet (hs_orb_borrowers = refs minus the owner's reference)
    std::atomic<int> refs{1};                 // the owner's reference (dropped by hs_orb_destroy) + one per communicator created on the handle; whoever drops the last one frees it
    hipStream_t stream = nullptr;
    std::string err;
    uint16_t taps[7];
    HsKnobs knobs{};                   // the handle's HS_* environment knobs, read once in hs_orb_create (hs_read_knobs has the table); split_mode is also set by hs_orb_set_split
    uint32_t fast_epoch = 0;           // FAST launches on this workspace so far (selects the work-queue counter set)
    hipStream_t s_aux = nullptr; hipEvent_t ev_sfork = nullptr, ev_sjoin = nullptr;      // the second launch sequence of the split and its fences
    bool fast_taps = false;            // every tap fits a byte and the 16-bit row sums cannot saturate
    // ORBExtractor ctor tables (ORBExtractor.cpp:86-118)
    std::vector<float> scale, inv_scale, sigma2, inv_sigma2;
    std::vector<int> quota;
    // Everything configure() builds for one frame size and batch capacity, and what the last call left behind that only holds for them.
    // free_geometry() is `geo = Geometry{}`: the buffers free themselves and w = h = batch_cap = 0 says that nothing is configured.
    struct Geometry {
        int w = 0, h = 0, batch_cap = 0;
        uint64_t plan_digest = 0;          // HsPlan::digest of the plan this geometry was made from (hs_debug_plan_digest)
        std::vector<HsLevel> lv;           // the levels, host copy of d_lv (empty: no plan since the last reset)
        std::vector<HsLevel> lv_n;         // the same levels with the NARROW FAST work items (grp_cells / ngroups / item_begin differ); device copy at d_lv + nlevels
        int last_batch = 0; HsImg0 last_img0{};      // the last extraction on this geometry: frames and where level 0 was (the hs_orb_debug_* readers)
        int last_pyr_launches = 0;         // kernel launches the pyramid stage of the last call really enqueued (hs_launch_pyramid's return value); 0 = no call yet
        int total_cells = 0, max_wcell = 1, max_hcell = 1;
        int fast_items = 0;                // FAST work items per image (HsLevel::item_begin)
        int fast_items_n = 0;              // narrow items per image; 0 = no narrow list (a cell wider than the narrow tile)
        uint64_t cand_img_stride = 0;      // candidate entries per image
        int sel_img_stride = 0;            // selection entries per image
        int max_kp = 0;
        HsBuf<HsFastItem> d_fast_items, d_fast_items_n;
        HsBuf<uint32_t> d_fast_ovf;
        HsBuf<uint8_t> d_pyr;
        HsBuf<int16_t> d_tables;
        HsBuf<uint8_t> d_qt_tabs;          // geometric-key tables of the count-domain quadtree (hs_plan.hip)
        // round 4: the FAST kernel computes the candidates' geometric keys and leaves their histogram + the best candidate per deepest cell in global
        // memory (HsFastQt, HsLevel::qt_hist_off): u16 key tables, the per-level records, the two arrays ([batch][stride]; all zero between calls:
        // the quadtree kernel zeroes what it consumes)
        HsBuf<uint16_t> d_qkeys; HsBuf<HsFastQt> d_fast_qt;
        HsBuf<uint32_t> d_qhist; HsBuf<unsigned long long> d_qbest; uint32_t qhist_stride = 0, qbest_stride = 0;
        HsBuf<uint8_t> d_qt_rects;         // qt_large: batch_cap * nlevels * hs_quadtree_large_scratch_bytes()
        bool keys_dirty = false;           // a keyed call was enqueued and did not reach its end (any error return of run_extract): d_qhist / d_qbest may hold stale keys -> zeroed before the next call
        HsBuf<uint8_t> d_pyr_tabs;         // tile / row records of the fused and chain pyramid kernels (HsPlan::pyr_tabs, made by hs_plan_pyramid.hip)
        std::vector<HsPyrFuse> pyr_fuse;   // [level]: kernel argument of the pair (level, level + 1) when it is fused
        HsBuf<uint8_t> d_pyr_cols;         // column records of the LDS-staged pyramid kernels (HsPlan::pyr_cols)
        std::vector<HsPyrFuseCols> pyr_fuse_cols; std::vector<HsPyrChainCols> pyr_chain_cols, pyr_deep_cols;   // [level]: the records of pyr_fuse / pyr_chain / pyr_deep (in d_pyr_cols)
        std::vector<const uint8_t*> pyr_level_cols;   // [level]: column records of a level made on its own (in d_pyr_cols)
        std::vector<HsPyrChain> pyr_deep;  // [level]: the small-batch plan — chains as long as the LDS allows (8 levels: all seven in ONE launch); valid = 0 where none starts
        std::vector<HsPyrChain> pyr_chain; // [level]: kernel argument of the chain launch that starts at this level (HsLevel::chain_n levels)
        HsBuf<uint2> d_cand; HsBuf<uint32_t> d_pts_xy, d_pts_sk; HsBuf<uint16_t> d_pt_node;
        HsBuf<int32_t> d_cand_count, d_sel_count, d_cell_count;
        HsBuf<uint32_t> d_sel;
        HsBuf<uint16_t> d_sel_perm;        // spatial order of every level's selection (describe stage)
    } geo;
    HsBuf<HsLevel> d_lv;               // [2][HS_MAX_LEVELS]: lv, then lv_n
    HsBuf<uint16_t> d_taps;
    bool qt_large = false;             // a level's quota + 8 exceeds HS_QT_MAX_NODES (up to HS_QT_LARGE_NODES): the quadtree kernel's large-list instance, rectangles in d_qt_rects
    bool qt_small_ok = false;          // HS_QT_SMALL=1 and every level's list (quota + 8 nodes) fits the quadtree kernel's small instance (two workgroups per CU)
    bool keep_points = false;          // hs_orb_set_debug(h, 1): the quadtree kernel also gathers the candidates into the dense point arrays (hs_orb_debug_candidates reads them)
    // staging for the host-pointer entry points (regrown behind a drained `stream`)
    HsFrameStaging in;
    HsBuf<uint8_t> d_out;              // one block [counts | keypoints | descriptors] (out_layout), so that the results come back in ONE device-to-host copy
    HsStereoOut st;
    HsBuf<int32_t> d_strip_count; HsBuf<HsStripEntry> d_strip_list;      // two capacities: the counters (pairs * strips) and the lists (pairs * strips * cap) grow independently
    // persistent staging of hs_stereo_match (host-pointer call): device keypoints / descriptors / counts and one pinned host block
    HsBuf<hs_keypoint> d_sm_kps; HsBuf<uint8_t> d_sm_desc; HsBuf<int32_t> d_sm_n;
    HsPinned<uint8_t> h_pin;
    // hs_orb_extract_batch (host-pointer call): one pinned block the three outputs come back into
    HsPinned<uint8_t> h_pin_out;
    // (the two below outlive a reconfiguration: the matcher has no geometry, and the published results live in d_out / a slot's block, not in the workspace)
    int last_qt_launches = 1;          // launches of stage 2 in the last call: 2 when the upper levels ran on the level instance (run_extract)
    int last_stereo_launches = 2;      // launches of stage 4 in the last stereo call: strips + match (run_stereo) or match only (the front end with the strips inside the describe launch)
    // where the last host-pointer extraction (hs_orb_extract[_batch], hs_orb_wait) left its results on the DEVICE: what hs_frame_publish keeps
    const hs_keypoint* pub_kps = nullptr; const uint8_t* pub_desc = nullptr; int pub_cap = 0, pub_batch = 0;
    // grow-only scratch arena of the host-pointer entry points (HsStage, hs_internal.h)
    HsBuf<uint8_t> d_scratch;
    // pipelined host ingest (hs_orb_submit_batch / hs_orb_wait): two staging slots, a copy-in and a copy-out stream next to the compute stream
    struct IngestSlot {
        HsFrameStaging in;                 // frames of the batch in HBM (regrown while the slot is idle: nothing to wait for)
        HsBuf<uint8_t> d_out;              // [counts | keypoints | descriptors | uRight | depth] in HBM (out_layout)
        HsPinned<uint8_t> h_out;           // the same block in page-locked host memory
        hipEvent_t ev_in = nullptr, ev_done = nullptr, ev_out = nullptr;
        int32_t ticket = 0; bool busy = false;
        int batch = 0, pairs = 0, cap = 0;
    } slot[2];
    hipStream_t s_in = nullptr, s_out = nullptr;
    int32_t next_ticket = 1;
    // second lane (hs_orb_set_lanes): a child handle with its own workspace and stream, fenced against the caller's stream by two events
    hs_orb* lane2 = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // stage profiling: events[i] marks the start of stage prof_stage[i]; the event after the last stage has stage -1
    bool prof = false;
    std::vector<hipEvent_t> ev_pool; size_t ev_used = 0;
    std::vector<int> prof_stage;
};

namespace {

inline int cv_round_f(float v) { return (int)nearbyintf(v); }           // cvRound: round half to even

// record "stage `stage` starts here" (stage -1 closes the previous one) when profiling is on
void mark(hs_orb* h, int stage, hipStream_t s)
{
    if (!h->prof) return;
    if (h->ev_used == h->ev_pool.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return; h->ev_pool.push_back(e); }
    (void)hipEventRecord(h->ev_pool[h->ev_used++], s);
    h->prof_stage.push_back(stage);
}

// nothing is configured any more (w = h = batch_cap = 0) and the buffers of the geometry are freed: a failed configure() must not leave a
// geometry that the early exit would accept
void free_geometry(hs_orb* h) { h->geo = hs_orb::Geometry{}; }

// The plan's pointer fields hold byte offsets (hs_plan.h); these turn them into addresses, in one place per buffer.  "None" is decided by
// what the record is, never by a zero offset: level 1 sits at offset 0 of an image's pyramid while base == nullptr means level 0.
template <class T> void relocate(T*& p, const void* base) { p = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + reinterpret_cast<uintptr_t>(p)); }
void relocate_levels(std::vector<HsLevel>& lv, const hs_orb::Geometry& g)
{
    for (size_t l = 0; l < lv.size(); l++) {
        HsLevel& V = lv[l];
        if (l > 0) { relocate(V.base, g.d_pyr.p); relocate(V.xofs, g.d_tables.p); relocate(V.ialpha, g.d_tables.p); relocate(V.yofs, g.d_tables.p); relocate(V.ibeta, g.d_tables.p); }
        if (V.qt_ytab) { relocate(V.qt_xtab, g.d_qt_tabs.p); relocate(V.qt_ytab, g.d_qt_tabs.p); }      // (the y table follows the x table: its offset is never 0)
    }
}
void relocate_pyramid(hs_orb::Geometry& g)
{
    for (std::vector<HsPyrChain>* plan : { &g.pyr_chain, &g.pyr_deep })
        for (size_t l = 0; l < plan->size(); l++) {
            HsPyrChain& C = (*plan)[l];
            if (!C.valid) continue;
            if (l > 1) relocate(C.sbase, g.d_pyr.p);                // a chain that starts at level 1 reads the caller's frames
            for (int i = 0; i < C.nstage; i++) {
                HsPyrStage& S = C.st[i];
                relocate(S.base, g.d_pyr.p); relocate(S.xt, g.d_tables.p);
                relocate(S.rows, g.d_pyr_tabs.p); relocate(S.tx, g.d_pyr_tabs.p); relocate(S.ty, g.d_pyr_tabs.p);
            }
        }
    for (size_t l = 0; l < g.pyr_fuse.size(); l++) {
        HsPyrFuse& F = g.pyr_fuse[l];
        if (!F.valid) continue;
        if (l > 1) relocate(F.sbase, g.d_pyr.p);
        relocate(F.abase, g.d_pyr.p); relocate(F.bbase, g.d_pyr.p); relocate(F.xtA, g.d_tables.p); relocate(F.xtB, g.d_tables.p);
        relocate(F.rowA, g.d_pyr_tabs.p); relocate(F.rowB, g.d_pyr_tabs.p); relocate(F.xt, g.d_pyr_tabs.p); relocate(F.yt, g.d_pyr_tabs.p);
    }
    // the column records: every place that was given one (a null offset cannot occur: word 0 of the blob is padding)
    for (HsPyrFuseCols& K : g.pyr_fuse_cols) { if (K.a) relocate(K.a, g.d_pyr_cols.p); if (K.b) relocate(K.b, g.d_pyr_cols.p); }
    for (std::vector<HsPyrChainCols>* plan : { &g.pyr_chain_cols, &g.pyr_deep_cols })
        for (HsPyrChainCols& K : *plan) for (const uint8_t*& c : K.st) if (c) relocate(c, g.d_pyr_cols.p);
    for (size_t l = 1; l < g.pyr_level_cols.size(); l++) relocate(g.pyr_level_cols[l], g.d_pyr_cols.p);
}
template <class T, class V> hipError_t upload(const HsBuf<T>& d, const std::vector<V>& v)
{
    return v.empty() ? hipSuccess : hipMemcpy(d.p, v.data(), v.size() * sizeof(V), hipMemcpyHostToDevice);
}

// (Re)build per-level geometry, tables and workspace for batches of `batch` frames of w x h: plan on the host (hs_plan.hip), then allocate
// from the plan's sizes, upload its arrays and turn its offsets into addresses.
int configure_impl(hs_orb* h, int w, int hh, int batch);
int configure(hs_orb* h, int w, int hh, int batch)
{
    if (w == h->geo.w && hh == h->geo.h && batch <= h->geo.batch_cap) return HS_OK;
    if (w < 1 || hh < 1 || w > 16384 || hh > 16384 || batch < 1 || batch > 65535)
        return hs_fail(h, HS_ERR_INVALID, "image size / batch out of range");
    const int rc = configure_impl(h, w, hh, batch);
    if (rc != HS_OK) free_geometry(h);             // partial allocations of a failed attempt go away; the handle stays usable
    return rc;
}
int configure_impl(hs_orb* h, int w, int hh, int batch)
{
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    free_geometry(h);                  // also un-configures: every failure return below leaves w = h = batch_cap = 0
    hs_orb::Geometry& g = h->geo;
    const int L = h->p.nlevels;
    HsPlan P; std::string refusal;
    const HsPlanInput in{ &h->p, h->inv_scale.data(), h->scale.data(), h->quota.data(), &h->knobs, h->qt_large, w, hh };
    const int rc = hs_plan_geometry(in, P, refusal);
    if (rc != HS_OK) return hs_fail(h, rc, refusal);
    g.total_cells = P.total_cells; g.max_wcell = P.max_wcell; g.max_hcell = P.max_hcell; g.fast_items = P.fast_items; g.fast_items_n = P.fast_items_n;
    g.cand_img_stride = P.cand_img_stride; g.sel_img_stride = P.sel_img_stride; g.max_kp = P.max_kp;
    g.qhist_stride = P.qhist_stride; g.qbest_stride = P.qbest_stride; g.plan_digest = P.digest;
    g.lv = std::move(P.lv); g.lv_n = std::move(P.lv_n);
    g.pyr_fuse = std::move(P.pyr_fuse); g.pyr_chain = std::move(P.pyr_chain); g.pyr_deep = std::move(P.pyr_deep);
    g.pyr_fuse_cols = std::move(P.pyr_fuse_cols); g.pyr_chain_cols = std::move(P.pyr_chain_cols); g.pyr_deep_cols = std::move(P.pyr_deep_cols);
    g.pyr_level_cols = std::move(P.pyr_level_cols);

    // ---- allocate: every size is the plan's per-image figure times `batch`, with a floor that keeps an empty buffer addressable
    HIP_TRY(h, g.d_pyr.grow(std::max<size_t>(P.pyr_per_img * batch, 256)));
    HIP_TRY(h, g.d_tables.grow(std::max<size_t>(P.tables.size(), 256 / sizeof(int16_t))));
    const size_t ce = std::max<uint64_t>(g.cand_img_stride * batch, 64);
    HIP_TRY(h, g.d_cand.grow(ce));
    HIP_TRY(h, g.d_pts_xy.grow(ce));
    HIP_TRY(h, g.d_pts_sk.grow(ce));
    HIP_TRY(h, g.d_pt_node.grow(ce));
    if (h->qt_large) HIP_TRY(h, g.d_qt_rects.grow((size_t)batch * L * hs_quadtree_large_scratch_bytes()));
    HIP_TRY(h, g.d_cell_count.grow(std::max<size_t>((size_t)g.total_cells * batch, 64 / 4)));
    HIP_TRY(h, g.d_cand_count.grow((size_t)batch * L));
    HIP_TRY(h, g.d_sel_count.grow((size_t)batch * L));
    HIP_TRY(h, g.d_sel.grow(std::max<size_t>((size_t)g.sel_img_stride * batch * 3, 64 / 4)));          // 12 bytes per selection entry
    HIP_TRY(h, g.d_sel_perm.grow(std::max<size_t>((size_t)g.sel_img_stride * batch, 64 / 2)));
    HIP_TRY(h, g.d_qt_tabs.grow(std::max<size_t>(P.qt_tabs.size() + 16, 256)));
    HIP_TRY(h, g.d_qkeys.grow(std::max<size_t>(P.qkeys.size() + 16 / 2, 256 / 2)));
    HIP_TRY(h, g.d_fast_qt.grow(HS_MAX_LEVELS));
    HIP_TRY(h, g.d_qhist.grow(std::max<size_t>((size_t)g.qhist_stride * batch, 256 / 4)));
    HIP_TRY(h, g.d_qbest.grow(std::max<size_t>((size_t)g.qbest_stride * batch, 256 / 8)));
    HIP_TRY(h, g.d_pyr_tabs.grow(std::max<size_t>(P.pyr_tabs.size() * 8, 256)));
    HIP_TRY(h, g.d_pyr_cols.grow(std::max<size_t>(P.pyr_cols.size() * 8, 256)));
    HIP_TRY(h, g.d_fast_items.grow(P.items.size()));
    HIP_TRY(h, g.d_fast_items_n.grow(P.items_n.size()));
    HIP_TRY(h, g.d_fast_ovf.grow(std::max<size_t>(hs_fast_overflow_bytes(h->knobs, g.max_hcell, g.fast_items, g.fast_items_n, batch), 256) / 4));      // (a multiple of 4 bytes)

    // ---- offsets -> addresses.  The FAST items were built by the plan from the levels' offsets (hs_plan_fast.hip copies HsLevel::base), so
    // they are relocated here by HsFastItem::level rather than rebuilt from the relocated levels.
    relocate_levels(g.lv, g); relocate_levels(g.lv_n, g);
    relocate_pyramid(g);
    for (size_t l = 0; l < P.fast_qt.size(); l++) if (P.fast_qt[l].enabled) { relocate(P.fast_qt[l].xkey, g.d_qkeys.p); relocate(P.fast_qt[l].ykey, g.d_qkeys.p); }
    for (std::vector<HsFastItem>* items : { &P.items, &P.items_n })
        for (HsFastItem& it : *items) if (it.level > 0) relocate(it.base, g.d_pyr.p);

    // ---- upload
    HIP_TRY(h, upload(g.d_tables, P.tables));
    HIP_TRY(h, upload(g.d_qt_tabs, P.qt_tabs));
    HIP_TRY(h, upload(g.d_qkeys, P.qkeys));
    HIP_TRY(h, upload(g.d_fast_qt, P.fast_qt));
    HIP_TRY(h, upload(g.d_pyr_tabs, P.pyr_tabs));
    HIP_TRY(h, upload(g.d_pyr_cols, P.pyr_cols));
    HIP_TRY(h, hipMemcpy(h->d_lv, g.lv.data(), sizeof(HsLevel) * L, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_lv + L, g.lv_n.data(), sizeof(HsLevel) * L, hipMemcpyHostToDevice));
    HIP_TRY(h, upload(g.d_fast_items, P.items));
    HIP_TRY(h, upload(g.d_fast_items_n, P.items_n));

    // ---- what the kernels expect to find zero (on the handle's stream: hipMemset on device memory is asynchronous to the host and runs on the NULL
    // stream, which the handle's non-blocking streams are not ordered with — a memset that lands after the first kernels would wipe what they wrote)
    HIP_TRY(h, hipMemsetAsync(g.d_qhist, 0, std::max<size_t>((size_t)g.qhist_stride * batch * 4, 256), h->stream));
    HIP_TRY(h, hipMemsetAsync(g.d_qbest, 0, std::max<size_t>((size_t)g.qbest_stride * batch * 8, 256), h->stream));
    HIP_TRY(h, hipMemsetAsync(g.d_fast_ovf, 0, 4 * HS_FAST_QUEUE_DWORDS * 4, h->stream));       // all four work-queue counter sets start at zero (stream-ordered before the first launch)
    HIP_TRY(h, hipStreamSynchronize(h->stream));     // the memsets above have landed whatever stream the caller's launches will use (configuration is rare: it allocates)
    g.w = w; g.h = hh; g.batch_cap = batch;      // configured only now
    return HS_OK;
}

// The handle's knobs of the environment: name, default, how the value is taken, meaning.  hs_read_knobs is their only reader and runs once, in
// hs_orb_create (a second lane's handle reads them again at its own creation).  INTEGRATION.md has the users' table of every HS_* variable.
enum KnobRule { K_ANY, K_FLAG /*v != 0*/, K_POSITIVE /*v > 0, else the default*/, K_NONNEG /*v >= 0, else the default*/, K_MIN2 /*v >= 2, else the default*/,
                K_TRISTATE /*unset (or INT_MIN) = -1, else v != 0*/ };
struct KnobRow { const char* name; int HsKnobs::* field; int def; KnobRule rule; const char* meaning; };
const KnobRow KNOBS[] = {
    { "HS_PYRAMID_NO_FUSE",     &HsKnobs::no_fuse,             0,             K_FLAG,     "one pyramid level per launch (parity tests of the unfused kernel)" },
    { "HS_PYRAMID_CHAIN",       &HsKnobs::chain_mode,          -1,            K_ANY,      "-1 = a three-level chain for the tail of an odd number of levels, 0 = never, 2 = chains for every fused pair too (parity tests)" },
    { "HS_PYRAMID_CHAIN2",      &HsKnobs::pyr_chain2,          0,             K_FLAG,     "HS_PYRAMID_PLAN: a 2 is a two-level chain launch, not the two-level kernel" },
    { "HS_PYRAMID_TBX_MAX",     &HsKnobs::pyr_tbx_max,         0,             K_ANY,      "cap on the level-B tile width of the two-level kernel (experiment: lane utilisation against time)" },
    { "HS_PYRAMID_DEEP_MAX",    &HsKnobs::deep_max_batch,      2,             K_ANY,      "calls of at most this many frames use the small-batch plan (0 = never)" },
    // (a workgroup's stages are a dependent sequence whose length goes with the rows per wave: more, flatter tiles shorten the launch although their halo rows cost more work)
    { "HS_PYRAMID_DEEP_ROWS",   &HsKnobs::deep_rows,           8,             K_MIN2,     "rows of the LAST level per tile in the small-batch plan" },
    { "HS_FAST_ORDER",          &HsKnobs::fast_order,          1,             K_ANY,      "order of an image's FAST work items: 1 = reduced levels deepest first, level 0 last; 0 = level 0 first (the order until round 3); 2 = reduced levels interleaved, level 0 last" },
    { "HS_FAST_PCAP",           &HsKnobs::fast_pcap,           0,             K_ANY,      "tuning: cap on the FAST kernel's list length" },
    { "HS_FAST_LIST_MIN",       &HsKnobs::fast_list_min,       0,             K_ANY,      "tuning: list entries the tallest item must keep (decides the workgroups per CU; 1024 = round 4's layout)" },
    { "HS_FAST_TEST_SMALL_LISTS", &HsKnobs::fast_small_lists,  0,             K_FLAG,     "parity tests: force the spill paths" },
    { "HS_FAST_WG_PER_CU",      &HsKnobs::fast_wg_per_cu,      0,             K_ANY,      "tuning: workgroups per CU" },
    { "HS_FAST_TEST_SCAN_B",    &HsKnobs::fast_scan_b,         0,             K_FLAG,     "parity tests: NMS from the score tile" },
    { "HS_FAST_IMAGE_MAJOR",    &HsKnobs::fast_image_major,    0,             K_FLAG,     "tuning / parity tests: the work units image-major whatever the batch" },
    { "HS_FAST_NQ",             &HsKnobs::fast_nq,             0,             K_ANY,      "tuning / parity tests: at most this many work queues (8, 16, 32)" },
    { "HS_FAST_COLS",           &HsKnobs::fast_cols,           0,             K_ANY,      "tuning / parity tests: 32 / 64 = narrow / wide items whatever the batch (default: by batch)" },
    { "HS_FAST_NARROW_MAX",     &HsKnobs::fast_narrow_max,     0,             K_ANY,      "tuning: narrow items for launches of at most this many (narrow) work items" },
    { "HS_FAST_NO_FOLD",        &HsKnobs::fast_no_fold,        0,             K_FLAG,     "tuning / parity tests: work queues even for launches of <= 2 units per workgroup" },
    { "HS_FAST_KEYS",           &HsKnobs::fast_keys,           1,             K_FLAG,     "0: the quadtree kernel gathers the candidates and computes the keys itself (the scheme until round 3)" },
    { "HS_FAST_KEYS_LEVELS",    &HsKnobs::fast_keys_levels,    HS_MAX_LEVELS, K_POSITIVE, "only the levels 0 .. n-1 get keys (tuning)" },
    { "HS_FAST_KEYS_MAX_BATCH", &HsKnobs::fast_keys_max_batch, 16,            K_NONNEG,   "calls of more frames than this run without the keys (see run_extract)" },
    { "HS_QT_POINT_DOMAIN",     &HsKnobs::qt_point_domain,     0,             K_FLAG,     "the quadtree's general point-domain passes only (parity tests of the fallback)" },
    // (measured at 32 / 64 pairs per call the two-per-CU instance is SLOWER (quadtree 0.0631 against 0.0606 ms, 0.1198 against 0.1117): without the points in LDS every
    //  sweep goes through L2, which costs a workgroup more than sharing the CU buys.  Kept as a parity / tuning variant: tests/test_gpu_parity.py runs it.)
    { "HS_QT_SMALL",            &HsKnobs::qt_small,            0,             K_FLAG,     "the quadtree kernel's small instance (two workgroups per CU) where every level's list fits it" },
    { "HS_QT_SMALL_FROM",       &HsKnobs::qt_small_from,       -1,            K_ANY,      "calls of more than 256 (image, level) workgroups without the FAST keys: the levels from this one run on the quadtree kernel's level instance (eight waves, four workgroups per CU) where the plan allows it (hs_quadtree_small_from); -1 = from the plan's first such level, nlevels = off" },
    { "HS_QT_SMALL_THREADS",    &HsKnobs::qt_small_threads,    512,           K_ANY,      "tuning / parity tests: 256 = the level instance with four waves instead of eight" },
    { "HS_STEREO_FUSE",         &HsKnobs::stereo_fuse,         1,             K_FLAG,     "0: the stereo front end with a separate k_stereo_strips launch instead of the strips binned by an extra workgroup of the describe launch" },
    { "HS_STEREO_KPW",          &HsKnobs::stereo_kpw,          0,             K_ANY,      "tuning / parity tests: left keypoints per wavefront of the stereo matcher: 0 = by batch, 1 / 2 = k_stereo_match, 4 / 8 = k_stereo_match_compact, whatever the batch" },
    { "HS_EXTRACT_SPLIT",       &HsKnobs::split_mode,         -1,            K_TRISTATE, "1 = always run level 0's FAST + quadtree beside the pyramid, 0 = never, unset = for small batches (hs_orb_set_split overrides)" },
};
} // namespace
HsKnobs hs_read_knobs()
{
    HsKnobs k{};
    for (const KnobRow& r : KNOBS) {
        int& dst = k.*r.field;
        dst = r.def;
        const char* e = getenv(r.name);
        if (!e) continue;
        const int v = atoi(e);
        switch (r.rule) {
        case K_ANY: dst = v; break;
        case K_FLAG: dst = v != 0; break;
        case K_POSITIVE: if (v > 0) dst = v; break;
        case K_NONNEG: if (v >= 0) dst = v; break;
        case K_MIN2: if (v >= 2) dst = v; break;
        case K_TRISTATE: dst = v == INT_MIN ? -1 : (v != 0 ? 1 : 0); break;
        }
    }
    // HS_PYRAMID_PLAN (tuning): explicit chain lengths from level 1, e.g. "2,3,2"; parsed by the plan (hs_plan.hip: plan_pyramid)
    if (const char* e = getenv("HS_PYRAMID_PLAN")) { k.pyr_plan_set = true; k.pyr_plan = e; }
    return k;
}
namespace {

// The result block of a host-pointer extraction, on the device and in pinned host memory: [counts | keypoints | descriptors] of `batch` images
// of `cap` entries and, for a stereo ticket, [uRight | depth] of `pairs` left images.  Every piece starts on a multiple of 256 bytes.
struct OutLayout { size_t off_k, off_d, off_u, off_z, bytes; };
OutLayout out_layout(int batch, int cap, int pairs)
{
    OutLayout o;
    o.off_k = hs_up256((size_t)batch * 4);
    o.off_d = o.off_k + hs_up256((size_t)batch * cap * sizeof(hs_keypoint));
    const size_t desc = (size_t)batch * cap * HS_DESC_BYTES, ur = (size_t)pairs * cap * 4;
    o.off_u = o.off_z = o.bytes = o.off_d + desc;
    if (pairs > 0) { o.off_u = o.off_d + hs_up256(desc); o.off_z = o.off_u + hs_up256(ur); o.bytes = o.off_z + ur; }
    return o;
}

// A pinned result block goes to the caller's [batch][cap] arrays: only the entries that exist are copied (the counts clamped to [0, cap0], the
// capacity the block was laid out for); the rest of the caller's arrays is left untouched.  uRight / depth belong to the first `pairs` images.
void scatter_results(const uint8_t* blk, const OutLayout& o, int batch, int cap0, int pairs, hs_keypoint* kps, uint8_t* desc, int32_t* n, int cap, float* uRight, float* depth)
{
    memcpy(n, blk, (size_t)batch * 4);
    for (int i = 0; i < batch; i++) {
        const size_t cnt = (size_t)std::min(std::max(n[i], 0), cap0);
        memcpy(kps + (size_t)i * cap, blk + o.off_k + (size_t)i * cap0 * sizeof(hs_keypoint), cnt * sizeof(hs_keypoint));
        memcpy(desc + (size_t)i * cap * HS_DESC_BYTES, blk + o.off_d + (size_t)i * cap0 * HS_DESC_BYTES, cnt * HS_DESC_BYTES);
        if (i < pairs) {
            memcpy(uRight + (size_t)i * cap, blk + o.off_u + (size_t)i * cap0 * 4, cnt * 4);
            memcpy(depth + (size_t)i * cap, blk + o.off_z + (size_t)i * cap0 * 4, cnt * 4);
        }
    }
}

int ensure_stereo_strips(hs_orb* h, int pairs, int cap, int n_rows)
{
    if (n_rows > 65536) return hs_fail(h, HS_ERR_INVALID, "stereo: more than 65536 image rows");      // k_stereo_strips keeps one counter per 32 rows in LDS
    const size_t need_count = (size_t)pairs * hs_stereo_strips(n_rows);
    HIP_TRY(h, h->d_strip_count.grow(need_count, h->stream));
    HIP_TRY(h, h->d_strip_list.grow(need_count * (size_t)cap, h->stream));
    return HS_OK;
}

// `sf`: the stereo front end — the describe launch also bins the right images' keypoints into the matcher's strips (HsStripFuse, kernels_describe.hip)
int run_extract(hs_orb* h, HsImg0 img0, int batch, HsOut out, hipStream_t s, const HsStripFuse* sf = nullptr)
{
    const int L = h->p.nlevels;
    hs_orb::Geometry& g = h->geo;
    // Level 0 needs no pyramid.  For one or two LARGE frames the chain of launches is latency-bound (dependent pyramid launches, a FAST launch
    // whose duration is its slowest work item, the level-0 quadtree workgroup — 0.11 ms for a 4000 x 3000 frame): level 0's FAST + quadtree run
    // on a second stream BESIDE the pyramid and the other levels' FAST + quadtree, joined before the describe stage.  Same kernels, same
    // results.  Measured (profiles/README.md row "C4", profiles/r03_bench_lines.json -> c4; the same figures as include/hyslam_amd.h quotes for
    // hs_orb_set_split): the 4000 x 3000 "Imaging" extraction 0.413 ms unsplit -> 0.207 ms split (config C4: 2 592 -> 4 068 steps/s with both cameras
    // split); a 1080p pair gets SLOWER (0.132 -> 0.160 ms: the fork / join between the streams costs more than the overlap saves), 16 pairs too
    // (-7 %), hence the size rule.  Not with stage events (they would serialise the two sequences).  The two concurrent FAST launches rely on every
    // earlier launch of the handle having completed: a handle is driven from ONE stream at a time (include/hyslam_amd.h).
    const bool narrow = hs_fast_narrow(h->knobs, g.fast_items_n, batch);      // item width by batch
    // Keys by batch as well: the FAST kernel's two global atomics per candidate cost it 5 % at 16 pairs per call (0.162 -> 0.170 ms) and buy the
    // quadtree launch 4 us there (its 256 workgroups fill the chip either way); at one pair per call they cost 1 us and buy 10 (35.1 -> 24.8 us: the
    // level-0 workgroup no longer gathers 5 000 records on one CU).  Both arrays are zero between calls whatever the mode, so the mode may change per call.
    const HsPyrChain* const deep = (batch <= h->knobs.deep_max_batch && !g.pyr_deep.empty()) ? g.pyr_deep.data() : nullptr;      // the pyramid's small-batch plan
    const bool use_keys = h->knobs.fast_keys && g.d_fast_qt.p != nullptr && batch <= h->knobs.fast_keys_max_batch;
    // d_qhist / d_qbest are all zero between calls (the quadtree kernel zeroes what it consumes).  A call that fails anywhere between the keyed FAST
    // launch and its end — an event / stream call of the split path, a later launch — breaks that: the flag makes the NEXT call start from zeroed arrays.
    if (g.keys_dirty) {
        HIP_TRY(h, hipDeviceSynchronize());
        if (g.d_qhist) HIP_TRY(h, hipMemsetAsync(g.d_qhist, 0, (size_t)g.qhist_stride * g.batch_cap * 4, s));
        if (g.d_qbest) HIP_TRY(h, hipMemsetAsync(g.d_qbest, 0, (size_t)g.qbest_stride * g.batch_cap * 8, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        g.keys_dirty = false;
    }
    if (use_keys) g.keys_dirty = true;                          // cleared at the end of a call that enqueued everything without error
    const std::vector<HsLevel>& lvh = narrow ? h->geo.lv_n : h->geo.lv;
    const HsLevel* const d_lv = h->d_lv + (narrow ? L : 0);
    const HsFastItem* const d_items = narrow ? g.d_fast_items_n.p : g.d_fast_items.p;
    const int n_items = narrow ? g.fast_items_n : g.fast_items;
    const int items0 = lvh[0].ngroups * lvh[0].nrows, first0 = lvh[0].item_begin;      // work items of level 0: the LAST items0 of the item list
    const bool split = !h->prof && L > 1 && items0 > 0 && items0 < n_items && (h->knobs.split_mode == 1 || (h->knobs.split_mode < 0 && batch <= 2 && (size_t)g.w * (size_t)g.h * (size_t)batch >= 6000000));
    auto fast = [&](int item_first, int item_count, int spill_slot, hipStream_t st) -> int {
        // launch N uses work-queue counter set N & 3 and relies on launch N - 2 having zeroed it: the epoch advances only when a launch was
        // enqueued without error; after a failed launch all sets are zeroed again so that the next one starts from a known state
        const HsFastLaunch plan = hs_fast_launch_plan(h->knobs, g.max_hcell, g.fast_items, g.fast_items_n, batch, item_first, item_count, spill_slot);
        const bool launched = hs_launch_fast(plan, d_items, img0, h->p.fast_threshold, g.d_cand, g.d_cell_count, g.cand_img_stride, g.total_cells, g.d_fast_ovf, h->fast_epoch,
                                             use_keys ? g.d_fast_qt.p : nullptr, g.d_qhist, g.d_qbest, g.qhist_stride, g.qbest_stride, st);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            (void)hipDeviceSynchronize();
            (void)hipMemsetAsync(g.d_fast_ovf, 0, 4 * HS_FAST_QUEUE_DWORDS * 4, h->stream);
            if (g.d_qhist) (void)hipMemsetAsync(g.d_qhist, 0, (size_t)g.qhist_stride * g.batch_cap * 4, h->stream);      // a launch that died half-way may have left keys behind
            if (g.d_qbest) (void)hipMemsetAsync(g.d_qbest, 0, (size_t)g.qbest_stride * g.batch_cap * 8, h->stream);
            (void)hipStreamSynchronize(h->stream);
            return hs_fail(h, HS_ERR_HIP, std::string("FAST launch: ") + hipGetErrorString(e));
        }
        if (launched) h->fast_epoch++;
        return HS_OK;
    };
    auto quadtree = [&](int level_first, int level_count, hipStream_t st, int level_mode = 0) {
        hs_launch_quadtree(d_lv, L, batch, g.total_cells, g.d_cand, g.d_cell_count, g.cand_img_stride,
                           g.d_pts_xy, g.d_pts_sk, g.d_pt_node, g.d_cand_count, g.d_sel, g.d_sel_count, g.sel_img_stride, g.d_sel_perm, h->knobs.qt_point_domain ? 1 : 0,
                           level_first, level_count, use_keys ? g.d_qhist.p : nullptr, g.d_qbest, g.qhist_stride, g.qbest_stride, h->keep_points ? 1 : 0,
                           level_mode ? level_mode : (h->qt_large ? 2 : (h->qt_small_ok ? 1 : 0)), g.d_qt_rects, st);
    };
    // A launch of more than 256 workgroups runs in rounds of one 16-wave workgroup per CU whatever the level holds: the levels from `qt_from`
    // (all of them small enough for it: hs_quadtree_small_from) go to the level instance (eight waves) in a launch of their own, four workgroups per CU.
    // Not with the FAST keys (their histogram is one level deeper than that instance's pyramid) and not on a large-list handle.
    // Whether that pays goes by the rounds of 256 the single launch needs: the levels below qt_from still run in rounds and the level launch costs
    // about one more, so the default (HS_QT_SMALL_FROM unset) splits only where at least two rounds go away.  Measured at 1080p, k = 2: 128 frames
    // (4 rounds -> 1 + the level launch) 0.112 -> 0.076 ms; 64 frames (2 rounds -> 1 + the level launch) 0.061 -> 0.071 ms, hence not there.
    // A level given in HS_QT_SMALL_FROM forces the split for every call of more than 256 workgroups.
    int qt_from = L;
    if (!use_keys && !h->qt_large && !h->qt_small_ok && (long long)L * batch > 256) {
        const int k = hs_quadtree_small_from(lvh.data(), L);
        auto rounds = [&](int levels) { return ((long long)levels * batch + 255) / 256; };
        if (h->knobs.qt_small_from >= 0) qt_from = std::min(L, std::max(h->knobs.qt_small_from, k));
        else if (rounds(L) - rounds(k) >= 2) qt_from = k;
    }
    const int qt_level_mode = h->knobs.qt_small_threads == 256 ? 3 : 4;
    h->last_qt_launches = 1;
    if (split) {
        if (!h->s_aux) {
            HIP_TRY(h, hipStreamCreateWithFlags(&h->s_aux, hipStreamNonBlocking));
            HIP_TRY(h, hipEventCreateWithFlags(&h->ev_sfork, hipEventDisableTiming));
            HIP_TRY(h, hipEventCreateWithFlags(&h->ev_sjoin, hipEventDisableTiming));
        }
        HIP_TRY(h, hipEventRecord(h->ev_sfork, s));                           // everything enqueued on s so far (the frames' upload, the previous call) comes first
        HIP_TRY(h, hipStreamWaitEvent(h->s_aux, h->ev_sfork, 0));
        int rc = fast(first0, items0, 1, h->s_aux);
        if (rc != HS_OK) return rc;
        quadtree(0, 1, h->s_aux);
        HIP_TRY(h, hipEventRecord(h->ev_sjoin, h->s_aux));
        h->geo.last_pyr_launches = hs_launch_pyramid(h->d_lv, h->geo.lv.data(), g.pyr_fuse.data(), g.pyr_chain.data(), L, img0, batch, s, HsPyrCols{ g.pyr_fuse_cols.data(), g.pyr_chain_cols.data(), g.pyr_deep_cols.data(), g.pyr_level_cols.data() }, deep);
        rc = fast(0, n_items - items0, 0, s);
        if (rc != HS_OK) return rc;
        quadtree(1, L - 1, s);
        HIP_TRY(h, hipStreamWaitEvent(s, h->ev_sjoin, 0));
    } else {
        mark(h, 0, s);
        h->geo.last_pyr_launches = hs_launch_pyramid(h->d_lv, h->geo.lv.data(), g.pyr_fuse.data(), g.pyr_chain.data(), L, img0, batch, s, HsPyrCols{ g.pyr_fuse_cols.data(), g.pyr_chain_cols.data(), g.pyr_deep_cols.data(), g.pyr_level_cols.data() }, deep);
        mark(h, 1, s);
        const int rc = fast(0, n_items, 0, s);
        if (rc != HS_OK) return rc;
        mark(h, 2, s);
        quadtree(0, qt_from, s);                                          // (a range of no levels launches nothing)
        if (qt_from < L) quadtree(qt_from, L - qt_from, s, qt_level_mode);
        h->last_qt_launches = (qt_from > 0) + (qt_from < L);
    }
    mark(h, 3, s);
    hs_launch_describe(h->d_lv, L, img0, batch, g.d_sel, g.d_sel_count, g.d_sel_perm, g.sel_img_stride, g.max_kp,
                       h->d_taps, out, s, h->fast_taps, sf ? *sf : HsStripFuse{});
    mark(h, -1, s);
    HIP_TRY(h, hipGetLastError());
    g.keys_dirty = false;
    h->geo.last_batch = batch; h->geo.last_img0 = img0;
    return HS_OK;
}

// registers what the matchers read of a frame that comes as host arrays: keypoints, descriptors and, as a temporary, the grid that
// hs_launch_frame_grid builds from the keypoints
struct DevFrame { hs_keypoint* kps; uint8_t* desc; int8_t* cell; };
void stage_frame(HsStage& st, const hs_frame_view* F, DevFrame* o)
{
    st.in(&o->kps, F->n, F->kps); st.in(&o->desc, (size_t)F->n * 32, F->desc);
    st.temp(&o->cell, hs_frame_grid_bytes(std::max(F->n, 1)));
}

// Stage 4.  `binned`: the strips were binned by an extra workgroup of the describe launch (HsStripFuse, the stereo front end): one launch less.
// (Round 4 also built the median rejection into the matcher — each pair's last workgroup, found with a ticket counter,
// the three result arrays written through with agent-scope atomic stores so that no L2 write-back is needed: bit-exact, but the write-through
// stores cost more than the launch they save: 0.056 against 0.022 + 0.006 ms per 16 pairs, 10.0 against 4.8 + 4.8 us for one pair.  Dropped.)
void run_stereo(hs_orb* h, bool binned, const hs_keypoint* kL, const uint8_t* dL, const int32_t* nL, const hs_keypoint* kR, const uint8_t* dR,
                const int32_t* nR, int pairs, int cap, const hs_stereo_params& sp, float* ur, float* depth, hipStream_t s)
{
    mark(h, 4, s);
    h->last_stereo_launches = binned ? 1 : 2;
    if (binned) hs_launch_stereo_match_only_kpw(kL, dL, nL, kR, dR, nR, pairs, cap, sp, ur, depth, h->st.bd, h->d_strip_count, h->d_strip_list, h->knobs.stereo_kpw, s);
    else hs_launch_stereo_kpw(kL, dL, nL, kR, dR, nR, pairs, cap, sp, ur, depth, h->st.bd, h->d_strip_count, h->d_strip_list, h->knobs.stereo_kpw, s);
    mark(h, 5, s);
    hs_launch_stereo_median(nL, pairs, cap, ur, depth, h->st.bd, sp.th_high, h->d_strip_count, sp.n_rows, s);
    mark(h, -1, s);
}

// the stereo front end on a configured handle whose stereo buffers are large enough: extraction of the left and the right frames in ONE
// launch sequence (out.split of each), then the matcher.  HS_STEREO_FUSE (default): the describe launch also bins the right keypoints into the matcher's strips
int run_stereo_frontend(hs_orb* h, HsImg0 img0, HsOut out, const hs_stereo_params& sp, float* ur, float* depth, hipStream_t s)
{
    const int pairs = out.split;
    const HsStripFuse sf{ 1, sp.n_rows, hs_stereo_strips(sp.n_rows), 0, sp.size_ref, h->d_strip_count, h->d_strip_list };
    const int rc = run_extract(h, img0, 2 * pairs, out, s, h->knobs.stereo_fuse ? &sf : nullptr);
    if (rc != HS_OK) return rc;
    run_stereo(h, h->knobs.stereo_fuse, out.kps, out.desc, out.n, out.kps2, out.desc2, out.n2, pairs, out.cap, sp, ur, depth, s);
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

// The two-lane split of a batch (hs_orb_set_lanes(2), count >= 2): the first half runs on the handle and the caller's stream, the second half on the
// child handle's own stream, fenced by the fork / join events.  body(lane, first, count, stream) does the unsplit work of `count` items from `first`.
template <class Body> int run_lanes(hs_orb* h, hipStream_t s, int count, Body body)
{
    hs_orb* const child = h->lane2;
    const int c0 = count / 2;
    child->prof = h->prof;
    HIP_TRY(h, hipEventRecord(h->ev_fork, s));
    HIP_TRY(h, hipStreamWaitEvent(child->stream, h->ev_fork, 0));
    int rc = body(h, 0, c0, s);
    if (rc == HS_OK) {
        rc = body(child, c0, count - c0, child->stream);
        if (rc != HS_OK) h->err = child->err;
    }
    HIP_TRY(h, hipEventRecord(h->ev_join, child->stream));
    HIP_TRY(h, hipStreamWaitEvent(s, h->ev_join, 0));
    return rc;
}

} // namespace

// host-side facts of the current configuration (tests: tests/cpp/host_sanitize, tools): launches of the pyramid's standard / small-batch plan,
// FAST work items per image (wide / narrow), levels with quadtree keys, longest deep chain, its LDS bytes
void hs_debug_plan_summary(const hs_orb* h, int32_t* out /*[8]*/)
{
    for (int i = 0; i < 8; i++) out[i] = 0;
    if (!h || h->geo.lv.empty()) return;
    const int L = h->p.nlevels;
    out[0] = hs_pyramid_launch_count(h->geo.lv.data(), L);
    int deep_launches = 0, longest = 0, lds = 0;
    for (int l = 1; l < L; l++) {
        deep_launches++;
        if (l < (int)h->geo.pyr_deep.size() && h->geo.pyr_deep[l].valid) {
            const HsPyrChain& C = h->geo.pyr_deep[l];
            if (C.nstage > longest) { longest = C.nstage; lds = (int)hs_pyr_chain_lds((size_t)C.x_bytes, C.h_rows); }
            l += C.nstage - 1;
        } else if (h->geo.lv[l].chain_n > 0 && l + h->geo.lv[l].chain_n <= L) l += h->geo.lv[l].chain_n - 1;
        else if (h->geo.lv[l].fuse_tbx > 0 && l + 1 < L) l++;
    }
    out[1] = L > 1 ? deep_launches : 0; out[2] = h->geo.fast_items; out[3] = h->geo.fast_items_n;
    for (int l = 0; l < L; l++) out[4] += h->geo.lv[l].qt_hist_off != 0xFFFFFFFFu;
    out[5] = longest; out[6] = lds;
    if (L > 1 && !h->geo.pyr_deep.empty() && h->geo.pyr_deep[1].valid) out[7] = h->geo.pyr_deep[1].grid_x * h->geo.pyr_deep[1].grid_y;
}
// the pyramid plans of the current configuration as the launches get them: relocated, their tables uploaded (tests/cpp/test_pyramid_columns.cpp reads
// them through the stand-in runtime, where device memory is host memory)
void hs_debug_pyramid_plan(const hs_orb* h, HsDebugPyramidPlan* out)
{
    *out = HsDebugPyramidPlan{};
    if (!h || h->geo.w <= 0) return;
    out->nlevels = h->p.nlevels; out->lv = h->geo.lv.data();
    out->fuse = h->geo.pyr_fuse.data(); out->chain = h->geo.pyr_chain.data(); out->deep = h->geo.pyr_deep.data();
    out->cols = HsPyrCols{ h->geo.pyr_fuse_cols.data(), h->geo.pyr_chain_cols.data(), h->geo.pyr_deep_cols.data(), h->geo.pyr_level_cols.data() };
}
// the digest of the plan the current configuration was made from (hs_plan_digest); 0 = nothing is configured
uint64_t hs_debug_plan_digest(const hs_orb* h) { return h && h->geo.w > 0 ? h->geo.plan_digest : 0; }

// ---- workspace poisoning (hs_internal.h; hs_debug_poison below)
std::atomic<int> g_hs_poison{-1};
static std::atomic<long long> g_hs_poison_violations{0};
void hs_poison_violation() { g_hs_poison_violations.fetch_add(1, std::memory_order_relaxed); }
// hipMemset on device memory returns before the fill has run (NULL stream); the handles' streams do not wait for that stream, so the host does
hipError_t hs_poison_fill(void* p, size_t bytes, int byte)
{
    const hipError_t e = hipMemset(p, byte, bytes);
    return e != hipSuccess ? e : hipStreamSynchronize(nullptr);
}
// one workgroup per gap: the smallest arena offset in [begin, end) whose byte is not `byte` goes to first[gap] (left at all ones: none).  Reads only.
__global__ __launch_bounds__(256) void k_poison_check(const uint8_t* __restrict__ base, const HsPoisonGaps g, int byte, unsigned long long* __restrict__ first)
{
    const int gap = blockIdx.x;
    if (gap >= g.n) return;
    const unsigned long long e = g.end[gap];
    unsigned long long m = ~0ull;
    for (unsigned long long i = g.begin[gap] + threadIdx.x; i < e; i += 256)
        if (base[i] != (uint8_t)byte) { m = i; break; }
    if (m != ~0ull) atomicMin(first + gap, m);
}
void hs_launch_poison_check(const uint8_t* d_base, const HsPoisonGaps& gaps, int byte, unsigned long long* d_first, hipStream_t s)
{
    if (gaps.n <= 0) return;
    hipLaunchKernelGGL(k_poison_check, dim3(gaps.n), dim3(256), 0, s, d_base, gaps, byte, d_first);
}

// accessors for the other translation units of the library (declared in hs_internal.h)
void hs_set_error(hs_orb* h, const char* msg) { if (h) h->err = msg ? msg : ""; }
int hs_orb_device_of(const hs_orb* h) { return h ? h->device : 0; }
hipStream_t hs_orb_stream_of(const hs_orb* h) { return h ? h->stream : nullptr; }
// (the grow-only arena that HsStage, hs_internal.h, lays the host-pointer entry points' pieces out in)
uint8_t* hs_orb_scratch_of(hs_orb* h, size_t bytes, hipStream_t user)
{
    // a regrow frees the old block: whatever was laid out in it may still be in use by work queued on the handle's stream (the host-pointer calls)
    // or on `user`, the stream of the stage that claims now (a device form on the caller's stream).  Both are drained first; without a regrow: no wait
    const auto claim = [&]() -> int {
        if (bytes > h->d_scratch.cap && user != h->stream) HIP_TRY(h, hipStreamSynchronize(user));
        HIP_TRY(h, h->d_scratch.grow(bytes, h->stream));
        return HS_OK;
    };
    return claim() == HS_OK ? h->d_scratch.p : nullptr;
}

extern "C" {

const char* hs_version(void) { return HS_VERSION; }

const char* hs_status_string(int s)
{
    switch (s) {
    case HS_OK: return "ok";
    case HS_ERR_INVALID: return "invalid argument";
    case HS_ERR_HIP: return "HIP runtime error";
    case HS_ERR_CAPACITY: return "output capacity too small";
    case HS_ERR_NO_DEVICE: return "no usable device";
    case HS_ERR_POISON: return "workspace poison check failed";
    default: return "unknown status";
    }
}

int hs_device_count(int* count)
{
    if (!count) return HS_ERR_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { *count = 0; return HS_ERR_NO_DEVICE; }
    *count = n;
    return HS_OK;
}

void hs_orb_default_params(hs_orb_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->nfeatures = 1000; p->scale_factor = 1.2f; p->nlevels = 8; p->cell_px = 30;
    p->ini_th_fast = 20; p->min_th_fast = 4;
    p->fast_threshold = 20;      // ORBFinder's in-class default; setThreshold() never changes it (ORBFinder.cpp:58-60)
    static const uint16_t t[7] = { 18, 34, 49, 55, 49, 34, 18 };
    memcpy(p->blur_taps, t, sizeof(t));
}

int hs_orb_create(const hs_orb_params* p, int device, hs_orb** out)
{
    if (!p || !out) return HS_ERR_INVALID;
    *out = nullptr;
    if (p->nlevels < 1 || p->nlevels > HS_MAX_LEVELS || p->nfeatures < 1 || !(p->scale_factor > 1.0f) || p->cell_px < 8 ||
        p->fast_threshold < 0 || p->fast_threshold > 255)
        return HS_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev) return HS_ERR_NO_DEVICE;
    hs_orb* h = new hs_orb();
    h->p = *p; h->device = device;
    h->knobs = hs_read_knobs();
    bool zero = true; for (int k = 0; k < 7; k++) zero = zero && p->blur_taps[k] == 0;
    static const uint16_t def[7] = { 18, 34, 49, 55, 49, 34, 18 };
    for (int k = 0; k < 7; k++) h->taps[k] = zero ? def[k] : p->blur_taps[k];
    { uint32_t sum = 0; bool bytes = true; for (int k = 0; k < 7; k++) { sum += h->taps[k]; bytes = bytes && h->taps[k] <= 255; } h->fast_taps = bytes && sum * 255u <= 0xFFFFu; }

    // ORBExtractor::ORBExtractor (ORBExtractor.cpp:86-118); scaleFactor is a double member fed from a float setting
    const int L = p->nlevels;
    const double scaleFactor = p->scale_factor;
    h->scale.resize(L); h->inv_scale.resize(L); h->sigma2.resize(L); h->inv_sigma2.resize(L); h->quota.resize(L);
    h->scale[0] = 1.0f; h->sigma2[0] = 1.0f;
    for (int i = 1; i < L; i++) { h->scale[i] = (float)(h->scale[i - 1] * scaleFactor); h->sigma2[i] = h->scale[i] * h->scale[i]; }
    for (int i = 0; i < L; i++) { h->inv_scale[i] = 1.0f / h->scale[i]; h->inv_sigma2[i] = 1.0f / h->sigma2[i]; }
    float factor = (float)(1.0f / scaleFactor);
    float nDesired = p->nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)L));
    int sum = 0;
    for (int l = 0; l < L - 1; l++) { h->quota[l] = cv_round_f(nDesired); sum += h->quota[l]; nDesired *= factor; }
    h->quota[L - 1] = std::max(p->nfeatures - sum, 0);
    for (int l = 0; l < L; l++)
        if (h->quota[l] + 8 > HS_QT_LARGE_NODES) { delete h; return HS_ERR_INVALID; }      // (a level's quota above 3320: nFeatures beyond ~11 600 @1.4 / ~15 300 @1.2 with 8 levels)
    for (int l = 0; l < L; l++) if (h->quota[l] + 8 > HS_QT_MAX_NODES) h->qt_large = true;
    h->qt_small_ok = true;
    for (int l = 0; l < L; l++) if (h->quota[l] + 8 > hs_quadtree_small_nodes()) h->qt_small_ok = false;
    if (!h->knobs.qt_small) h->qt_small_ok = false;      // ... and only on request (HS_QT_SMALL, see hs_read_knobs)

    if (hipSetDevice(device) != hipSuccess) { delete h; return HS_ERR_NO_DEVICE; }
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        h->d_lv.grow(2 * HS_MAX_LEVELS) != hipSuccess ||
        h->d_taps.grow(8) != hipSuccess ||
        hipMemcpy(h->d_taps, h->taps, 14, hipMemcpyHostToDevice) != hipSuccess) {
        hs_orb_destroy(h);
        return HS_ERR_HIP;
    }
    *out = h;
    return HS_OK;
}

static void orb_destroy_now(hs_orb* h);
void hs_orb_destroy(hs_orb* h)
{
    if (!h) return;
    h->owned.store(false);
    if (h->refs.fetch_sub(1) == 1) orb_destroy_now(h);                   // else a communicator still uses the handle: the last hs_comm_destroy frees it
}
int hs_orb_borrowers(const hs_orb* h) { return h ? std::max(0, h->refs.load() - (h->owned.load() ? 1 : 0)) : 0; }
} // extern "C"
// hs_comm.hip: +1 when a communicator is created on the handle, -1 when it is destroyed (which also completes a deferred hs_orb_destroy)
void hs_orb_borrow(hs_orb* h, int delta)
{
    if (!h) return;
    if (h->refs.fetch_add(delta) + delta == 0) orb_destroy_now(h);
}
static void orb_destroy_now(hs_orb* h)
{
    hipSetDevice(h->device);
    if (h->lane2) { hs_orb_destroy(h->lane2); h->lane2 = nullptr; }
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ev_join) hipEventDestroy(h->ev_join);
    if (h->s_aux) { hipStreamSynchronize(h->s_aux); hipStreamDestroy(h->s_aux); }
    if (h->ev_sfork) hipEventDestroy(h->ev_sfork);
    if (h->ev_sjoin) hipEventDestroy(h->ev_sjoin);
    // every stream is drained before anything is freed; the buffers themselves go with the handle (HsBuf's destructor, in `delete h` below)
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->s_in) hipStreamSynchronize(h->s_in);
    if (h->s_out) hipStreamSynchronize(h->s_out);
    for (auto& sl : h->slot) {
        if (sl.ev_in) hipEventDestroy(sl.ev_in);
        if (sl.ev_done) hipEventDestroy(sl.ev_done);
        if (sl.ev_out) hipEventDestroy(sl.ev_out);
    }
    if (h->s_in) hipStreamDestroy(h->s_in);
    if (h->s_out) hipStreamDestroy(h->s_out);
    for (hipEvent_t e : h->ev_pool) hipEventDestroy(e);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}
extern "C" {

const char* hs_orb_last_error(const hs_orb* h) { return h ? h->err.c_str() : "null handle"; }
int hs_orb_get_levels(const hs_orb* h) { return h ? h->p.nlevels : 0; }
int hs_orb_get_device(const hs_orb* h) { return h ? h->device : -1; }
float hs_orb_get_scale_factor(const hs_orb* h) { return h ? (float)(double)h->p.scale_factor : 0.f; }

int hs_orb_get_scale_tables(const hs_orb* h, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2, int32_t* fpl)
{
    if (!h) return HS_ERR_INVALID;
    for (int i = 0; i < h->p.nlevels; i++) {
        if (scale) scale[i] = h->scale[i];
        if (inv_scale) inv_scale[i] = h->inv_scale[i];
        if (sigma2) sigma2[i] = h->sigma2[i];
        if (inv_sigma2) inv_sigma2[i] = h->inv_sigma2[i];
        if (fpl) fpl[i] = h->quota[i];
    }
    return HS_OK;
}

int hs_orb_max_keypoints(const hs_orb* h)
{
    if (!h) return 0;
    // DistributeOctTree stops at the first split that reaches N nodes: at most N+2 per level, or the
    // 4*nIni nodes of the unconditional first pass.  nIni depends on the frame; assume the widest supported.
    int n = 0;
    for (int l = 0; l < h->p.nlevels; l++) n += std::max(h->quota[l] + 4, 4 * 8 + 4);
    return std::max(n, h->geo.max_kp);          // a configured geometry (hs_orb_reserve / a previous extract) with more than 8 root nodes per level needs more
}

int hs_orb_reserve(hs_orb* h, int w, int h_px, int batch)
{
    if (!h) return HS_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    return configure(h, w, h_px, batch);
}

int hs_orb_extract_batch_device(hs_orb* h, const uint8_t* d_imgs, int batch, int w, int h_px,
                                size_t row_stride, size_t image_stride,
                                hs_keypoint* d_kps, uint8_t* d_desc, int32_t* d_n, int cap, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!d_imgs || !d_kps || !d_desc || !d_n || batch < 1 || row_stride < (size_t)w || cap < 1 || cap > 65535)
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (((uintptr_t)d_desc & 15) != 0 || (((uintptr_t)d_kps | (uintptr_t)d_n) & 3) != 0)
        return hs_fail(h, HS_ERR_INVALID, "output alignment: descriptors 16 bytes (they are written with 16-byte vector stores; hs_record_offsets pads for it), keypoints and counts 4");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = hs_stream_or(h, stream);
    const auto body = [&](hs_orb* q, int first, int count, hipStream_t qs) -> int {
        int rc = configure(q, w, h_px, count);
        if (rc != HS_OK) return rc;
        if (cap < q->geo.max_kp) return hs_fail(q, HS_ERR_CAPACITY, "cap < keypoints this frame size can produce; see hs_orb_max_keypoints");
        const uint8_t* const imgs = d_imgs + (size_t)first * image_stride;
        hs_keypoint* const k = d_kps + (size_t)first * cap; uint8_t* const d = d_desc + (size_t)first * cap * HS_DESC_BYTES;
        HsImg0 img0{ imgs, imgs, count, (uint64_t)row_stride, (uint64_t)image_stride };
        HsOut out{ k, d, d_n + first, k, d, d_n + first, count, cap };
        return run_extract(q, img0, count, out, qs);
    };
    return h->lane2 && batch >= 2 ? run_lanes(h, s, batch, body) : body(h, 0, batch, s);
}

namespace {
// Frames that come as host pointers, grey (pp == nullptr: w x h IS the level-0 size) or as the camera delivers them (pp: 1 / 3 / 4 channels at the
// camera's own size; ImageProcessing::PreProcessImg runs on the device between the upload and the pyramid): the sizes of their staging copies
struct FramePlan {
    int w, h, gw, gh;                      // the frames as they come; the grey level 0
    size_t pitch, per_img;                 // level-0 frames in HsFrameStaging::d_in: rows padded to a multiple of 64 bytes
    size_t row_bytes, rpitch, raw_img;     // what is uploaded: a row, and (camera frames, in d_raw) rows packed to a multiple of 4 bytes
};
int plan_frames(hs_orb* h, int w, int h_px, const hs_preprocess_params* pp, FramePlan* u)
{
    u->w = u->gw = w; u->h = u->gh = h_px;
    if (pp) hs_preprocess_out_size(w, h_px, pp->scale, &u->gw, &u->gh);
    if (u->gw < 1 || u->gh < 1) return hs_fail(h, HS_ERR_INVALID, "the camera scale reduces the frame to nothing (cv::resize asserts on an empty size)");
    u->pitch = ((size_t)u->gw + 63) & ~(size_t)63; u->per_img = u->pitch * u->gh;
    u->row_bytes = (size_t)w * (pp ? pp->channels : 1);
    u->rpitch = pp ? (u->row_bytes + 3) & ~(size_t)3 : 0; u->raw_img = u->rpitch * h_px;
    return HS_OK;
}

// grows the staging pair for `batch` frames (`drain`: the stream to drain before a regrow; nullptr: the pair is idle) and enqueues the uploads on
// the copy stream `s`.  The frames cross PCIe as they are, once.  Pageable frames go through the runtime's own staging path (measured: packing the
// rows into a pinned buffer on the calling thread first is SLOWER — one core copies 2 MB frames at ~10 GB/s, the runtime's staged copy moves them
// at more than twice that); page-locked frames (hs_host_alloc) go by DMA at link speed and the call returns at once.
// `linear`: a frame whose rows are contiguous may go as ONE linear copy.  The synchronous calls say yes; the ingest path says no: measured with
// pageable 1080p frames, two tickets in flight, the linear copy holds the submitting thread longer than the 2-D one (9 130 against 10 250 pairs/s).
int upload_frames(hs_orb* h, HsFrameStaging& st, const hipStream_t* drain, const FramePlan& u, bool camera, const uint8_t* const* imgs, int batch, size_t stride, bool linear, hipStream_t s)
{
    HIP_TRY(h, drain ? st.d_in.grow(u.per_img * batch, *drain) : st.d_in.grow(u.per_img * batch));
    if (camera) HIP_TRY(h, drain ? st.d_raw.grow(u.raw_img * batch, *drain) : st.d_raw.grow(u.raw_img * batch));
    uint8_t* const dst = camera ? st.d_raw.p : st.d_in.p;
    const size_t dp = camera ? u.rpitch : u.pitch, di = camera ? u.raw_img : u.per_img;
    for (int i = 0; i < batch; i++) {
        // a frame whose rows are as far apart as the staging copy's (width a multiple of 64, no padding: 1920 x 1080) is ONE linear copy
        if (linear && stride == dp && u.row_bytes == dp) HIP_TRY(h, hipMemcpyAsync(dst + di * i, imgs[i], di, hipMemcpyHostToDevice, s));
        else HIP_TRY(h, hipMemcpy2DAsync(dst + di * i, dp, imgs[i], stride, u.row_bytes, u.h, hipMemcpyHostToDevice, s));      // (rows with padding: the last row's padding need not exist in the caller's buffer)
    }
    return HS_OK;
}

// camera scale + grey on the compute stream `s`, from the uploaded frames into the level-0 frames
int preprocess_frames(hs_orb* h, const HsFrameStaging& st, const FramePlan& u, const hs_preprocess_params& pp, int batch, hipStream_t s)
{
    hs_launch_preprocess(st.d_raw, u.w, u.h, u.rpitch, u.raw_img, pp.channels, pp.rgb, pp.scale, st.d_in, u.gw, u.gh, u.pitch, u.per_img, 1, batch, s);
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

// the host-pointer extraction, shared by hs_orb_extract_batch (grey frames) and hs_orb_extract_camera_batch (pp != nullptr)
int extract_host_frames(hs_orb* h, const uint8_t* const* imgs, int batch, int w, int h_px, size_t stride, const hs_preprocess_params* pp,
                        hs_keypoint* kps, uint8_t* desc, int cap, int32_t* n, uint8_t* grey_out)
{
    HIP_TRY(h, hipSetDevice(h->device));
    h->pub_kps = nullptr; h->pub_desc = nullptr; h->pub_batch = 0;
    FramePlan u;
    int rc = plan_frames(h, w, h_px, pp, &u);
    if (rc == HS_OK) rc = configure(h, u.gw, u.gh, batch);
    if (rc != HS_OK) return rc;
    if (cap < h->geo.max_kp) return hs_fail(h, HS_ERR_CAPACITY, "cap < keypoints this frame size can produce; see hs_orb_max_keypoints");
    hipStream_t s = h->stream;
    const OutLayout o = out_layout(batch, cap, 0);
    HIP_TRY(h, h->d_out.grow(o.bytes, s));
    for (int i = 0; i < batch; i++) if (!imgs[i]) return hs_fail(h, HS_ERR_INVALID, "null image in batch");
    rc = upload_frames(h, h->in, &s, u, pp != nullptr, imgs, batch, stride, true, s);
    if (rc == HS_OK && pp) rc = preprocess_frames(h, h->in, u, *pp, batch, s);
    if (rc != HS_OK) return rc;
    int32_t* const d_n = reinterpret_cast<int32_t*>(h->d_out.p);
    hs_keypoint* const d_kps = reinterpret_cast<hs_keypoint*>(h->d_out + o.off_k); uint8_t* const d_desc = h->d_out + o.off_d;
    HsImg0 img0{ h->in.d_in, h->in.d_in, batch, (uint64_t)u.pitch, (uint64_t)u.per_img };
    HsOut out{ d_kps, d_desc, d_n, d_kps, d_desc, d_n, batch, cap };
    rc = run_extract(h, img0, batch, out, s);
    if (rc != HS_OK) return rc;
    // counts, keypoints and descriptors live in one device block: one copy into pinned memory, then the used part goes to the caller
    HIP_TRY(h, h->h_pin_out.grow(o.bytes, s));
    HIP_TRY(h, hipMemcpyAsync(h->h_pin_out, h->d_out, o.bytes, hipMemcpyDeviceToHost, s));
    // the grey frame the reference keeps beside the features (track_data.image = mImGray, ImageProcessing.cpp:60,108): tight rows, on request
    if (grey_out) HIP_TRY(h, hipMemcpy2DAsync(grey_out, (size_t)u.gw, h->in.d_in, u.pitch, (size_t)u.gw, (size_t)u.gh * batch, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    scatter_results(h->h_pin_out, o, batch, cap, 0, kps, desc, n, cap, nullptr, nullptr);
    h->pub_kps = d_kps; h->pub_desc = d_desc; h->pub_cap = cap; h->pub_batch = batch;
    return HS_OK;
}
}  // namespace

int hs_orb_extract_batch(hs_orb* h, const uint8_t* const* imgs, int batch, int w, int h_px, int stride,
                         hs_keypoint* kps, uint8_t* desc, int cap, int32_t* n)
{
    if (!h) return HS_ERR_INVALID;
    if (!n || batch < 1) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (w == 0 || h_px == 0 || !imgs) { for (int i = 0; i < batch; i++) n[i] = 0; return HS_OK; }   // ORBExtractor.cpp:499-500
    if (!kps || !desc || stride < w || cap < 1 || cap > 65535) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    return extract_host_frames(h, imgs, batch, w, h_px, (size_t)stride, nullptr, kps, desc, cap, n, nullptr);
}

void hs_preprocess_size(int w, int h_px, float scale, int32_t* ow, int32_t* oh)
{
    int a = 0, b = 0;
    hs_preprocess_out_size(w, h_px, scale, &a, &b);
    if (ow) *ow = a;
    if (oh) *oh = b;
}

static bool preprocess_params_ok(const hs_preprocess_params* pp)
{
    return pp && (pp->channels == 1 || pp->channels == 3 || pp->channels == 4) && pp->scale > 0.f && pp->scale <= 16.f;
}

int hs_preprocess_device(hs_orb* h, const uint8_t* d_src, int w, int h_px, size_t row_stride, size_t image_stride, int batch, const hs_preprocess_params* pp,
                         uint8_t* d_grey, size_t grey_row_stride, size_t grey_image_stride, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!preprocess_params_ok(pp) || !d_src || !d_grey || w < 1 || h_px < 1 || w > 32768 || h_px > 32768 || batch < 1 || row_stride < (size_t)w * pp->channels)
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    int gw, gh;
    hs_preprocess_out_size(w, h_px, pp->scale, &gw, &gh);
    if (gw < 1 || gh < 1 || gw > 16384 || gh > 16384) return hs_fail(h, HS_ERR_INVALID, "the scaled frame is empty or larger than 16384 px");
    if (grey_row_stride < (size_t)gw) return hs_fail(h, HS_ERR_INVALID, "grey_row_stride < scaled width");
    HIP_TRY(h, hipSetDevice(h->device));
    hs_launch_preprocess(d_src, w, h_px, row_stride, image_stride, pp->channels, pp->rgb, pp->scale, d_grey, gw, gh, grey_row_stride, grey_image_stride, 0, batch,
                         hs_stream_or(h, stream));
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_orb_extract_camera_batch(hs_orb* h, const uint8_t* const* imgs, int batch, int w, int h_px, size_t row_stride, const hs_preprocess_params* pp,
                                hs_keypoint* kps, uint8_t* desc, int cap, int32_t* n, uint8_t* grey_out)
{
    if (!h) return HS_ERR_INVALID;
    if (!n || batch < 1) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (w == 0 || h_px == 0 || !imgs) { for (int i = 0; i < batch; i++) n[i] = 0; return HS_OK; }   // ORBExtractor.cpp:499-500
    if (!preprocess_params_ok(pp) || !kps || !desc || w < 0 || h_px < 0 || w > 32768 || h_px > 32768 || row_stride < (size_t)w * pp->channels || cap < 1 || cap > 65535)
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    return extract_host_frames(h, imgs, batch, w, h_px, row_stride, pp, kps, desc, cap, n, grey_out);
}

int hs_orb_extract(hs_orb* h, const uint8_t* img, int w, int h_px, int stride,
                   hs_keypoint* kps, uint8_t* desc, int cap, int32_t* n)
{
    if (!h) return HS_ERR_INVALID;
    if (!n) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (!img || w == 0 || h_px == 0) { *n = 0; return HS_OK; }
    const uint8_t* one[1] = { img };
    return hs_orb_extract_batch(h, one, 1, w, h_px, stride, kps, desc, cap, n);
}

int hs_stereo_match_batch_device(hs_orb* h, const hs_keypoint* d_kpsL, const uint8_t* d_descL, const int32_t* d_nL,
                                 const hs_keypoint* d_kpsR, const uint8_t* d_descR, const int32_t* d_nR,
                                 int pairs, int cap, const hs_stereo_params* sp,
                                 float* d_uRight, float* d_depth, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!d_kpsL || !d_descL || !d_nL || !d_kpsR || !d_descR || !d_nR || !sp || !d_uRight || !d_depth ||
        pairs < 1 || pairs > 65535 || cap < 1 || cap > 65535)
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->st.grow((size_t)pairs * cap, h->stream));
    const int rc = ensure_stereo_strips(h, pairs, cap, sp->n_rows);
    if (rc != HS_OK) return rc;
    hipStream_t s = hs_stream_or(h, stream);
    run_stereo(h, false, d_kpsL, d_descL, d_nL, d_kpsR, d_descR, d_nR, pairs, cap, *sp, d_uRight, d_depth, s);
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

namespace {
// What the two single-pair stereo calls share.  The head: the handle's pinned block of `front` bytes + counts + [2][cap] results, and the matcher's buffers
int stereo_pair_buffers(hs_orb* h, size_t front, int cap, int n_rows)
{
    HIP_TRY(h, h->h_pin.grow(std::max<size_t>(front + 16 + 2 * (size_t)cap * 4, 1 << 18), h->stream));
    HIP_TRY(h, h->d_sm_n.grow(2));
    HIP_TRY(h, h->st.grow((size_t)cap, h->stream));
    return ensure_stereo_strips(h, 1, cap, n_rows);
}
// The tail: the counts go up through the pinned block (at `front`), the matcher runs on one pair of `cap` entries (behind the frames' `ready` events
// when the keypoints come from the frame cache) and uRight / depth of the nL left keypoints come back through the pinned block
int stereo_pair_tail(hs_orb* h, size_t front, int nL, int nR, const hs_keypoint* kL, const uint8_t* dL, const hs_keypoint* kR, const uint8_t* dR, int cap,
                     const hs_stereo_params& sp, hipEvent_t readyL, hipEvent_t readyR, float* uRight, float* depth)
{
    hipStream_t s = h->stream;
    int32_t* pn = reinterpret_cast<int32_t*>(h->h_pin + front); float* pout = reinterpret_cast<float*>(h->h_pin + front + 16);
    pn[0] = nL; pn[1] = nR;
    HIP_TRY(h, hipMemcpyAsync(h->d_sm_n, pn, 8, hipMemcpyHostToDevice, s));
    if (readyL) HIP_TRY(h, hipStreamWaitEvent(s, readyL, 0));
    if (readyR) HIP_TRY(h, hipStreamWaitEvent(s, readyR, 0));
    run_stereo(h, false, kL, dL, h->d_sm_n, kR, dR, h->d_sm_n + 1, 1, cap, sp, h->st.ur, h->st.depth, s);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(pout, h->st.ur, (size_t)nL * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(pout + cap, h->st.depth, (size_t)nL * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    memcpy(uRight, pout, (size_t)nL * 4);
    memcpy(depth, pout + cap, (size_t)nL * 4);
    return HS_OK;
}
}  // namespace

int hs_stereo_match(hs_orb* h, const hs_keypoint* kpsL, const uint8_t* descL, int nL,
                    const hs_keypoint* kpsR, const uint8_t* descR, int nR,
                    const hs_stereo_params* sp, float* uRight, float* depth)
{
    if (!h) return HS_ERR_INVALID;
    if (!sp || nL < 0 || nR < 0 || nL > 65535 || nR > 65535) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (nL == 0) return HS_OK;
    if (!kpsL || !descL || !uRight || !depth || (nR > 0 && (!kpsR || !descR))) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    const int cap = std::max(std::max(nL, nR), 1);
    hipStream_t s = h->stream;
    // persistent staging (grow-only): no allocation on the steady-state path.  Inputs go through one pinned block so that the five
    // H2D copies are real asynchronous DMAs; outputs come back into the same block.
    const size_t room = (size_t)2 * std::max(cap, 2048);      // left at [0, cap), right at [cap, 2 cap)
    HIP_TRY(h, h->d_sm_kps.grow(room, s));
    HIP_TRY(h, h->d_sm_desc.grow(room * HS_DESC_BYTES, s));
    const size_t kb = (size_t)cap * sizeof(hs_keypoint), db = (size_t)cap * HS_DESC_BYTES;
    const int rc = stereo_pair_buffers(h, 2 * kb + 2 * db, cap, sp->n_rows);
    if (rc != HS_OK) return rc;
    hs_keypoint* dk = h->d_sm_kps; uint8_t* dd = h->d_sm_desc;
    uint8_t* pk = h->h_pin; uint8_t* pd = pk + 2 * kb;
    memcpy(pk, kpsL, (size_t)nL * sizeof(hs_keypoint));
    if (nR) memcpy(pk + kb, kpsR, (size_t)nR * sizeof(hs_keypoint));
    memcpy(pd, descL, (size_t)nL * 32);
    if (nR) memcpy(pd + db, descR, (size_t)nR * 32);
    HIP_TRY(h, hipMemcpyAsync(dk, pk, 2 * kb, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(dd, pd, 2 * db, hipMemcpyHostToDevice, s));
    return stereo_pair_tail(h, 2 * kb + 2 * db, nL, nR, dk, dd, dk + cap, dd + (size_t)cap * 32, cap, *sp, nullptr, nullptr, uRight, depth);
}

int hs_stereo_frontend_batch_device(hs_orb* h, const uint8_t* d_left, const uint8_t* d_right, int pairs,
                                    int w, int h_px, size_t row_stride, size_t image_stride,
                                    hs_keypoint* d_kpsL, uint8_t* d_descL, int32_t* d_nL,
                                    hs_keypoint* d_kpsR, uint8_t* d_descR, int32_t* d_nR, int cap,
                                    const hs_stereo_params* sp, float* d_uRight, float* d_depth, void* stream)
{
    // The reference runs two ORBExtractor instances side by side (ImageProcessing.cpp:82-83); here the left and
    // right frames of all pairs go through ONE launch sequence (images [0,pairs) = left, [pairs,2*pairs) = right).
    if (!h) return HS_ERR_INVALID;
    if (!d_left || !d_right || !d_kpsL || !d_descL || !d_nL || !d_kpsR || !d_descR || !d_nR || !sp || !d_uRight || !d_depth ||
        pairs < 1 || 2 * pairs > 65535 || row_stride < (size_t)w || cap < 1 || cap > 65535)
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if ((((uintptr_t)d_descL | (uintptr_t)d_descR) & 15) != 0 || (((uintptr_t)d_kpsL | (uintptr_t)d_kpsR | (uintptr_t)d_nL | (uintptr_t)d_nR | (uintptr_t)d_uRight | (uintptr_t)d_depth) & 3) != 0)
        return hs_fail(h, HS_ERR_INVALID, "output alignment: descriptors 16 bytes (they are written with 16-byte vector stores), everything else 4");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = hs_stream_or(h, stream);
    const auto body = [&](hs_orb* q, int first, int count, hipStream_t qs) -> int {
        int rc = configure(q, w, h_px, 2 * count);
        if (rc != HS_OK) return rc;
        if (cap < q->geo.max_kp) return hs_fail(q, HS_ERR_CAPACITY, "cap < keypoints this frame size can produce; see hs_orb_max_keypoints");
        HIP_TRY(q, q->st.grow((size_t)count * cap, q->stream));
        rc = ensure_stereo_strips(q, count, cap, sp->n_rows);
        if (rc != HS_OK) return rc;
        const size_t io = (size_t)first * image_stride, ko = (size_t)first * cap;
        HsImg0 img0{ d_left + io, d_right + io, count, (uint64_t)row_stride, (uint64_t)image_stride };
        HsOut out{ d_kpsL + ko, d_descL + ko * HS_DESC_BYTES, d_nL + first, d_kpsR + ko, d_descR + ko * HS_DESC_BYTES, d_nR + first, count, cap };
        return run_stereo_frontend(q, img0, out, *sp, d_uRight + ko, d_depth + ko, qs);
    };
    // two lanes: each handles half of the pairs end to end (extract L+R, match) on its own stream
    return h->lane2 && pairs >= 2 ? run_lanes(h, s, pairs, body) : body(h, 0, pairs, s);
}

/* ---- pipelined host ingest ----
 * The reference feeds its extractor from host memory through a bounded queue: System::TrackStereo pushes frames and throttles when more than two
 * are waiting (src/main/System.cc:194-196), ImageProcessing pops, extracts, matches and pushes the features on (src/main/ImageProcessing.cpp:69-116).
 * Here: submit(i+1) copies its frames in on the copy-in stream WHILE the kernels of batch i run on the compute stream and the results of batch i
 * leave on the copy-out stream; two staging slots, so at most two tickets are in flight — the same bound as the reference's queue. */
int hs_host_alloc(size_t bytes, void** out)
{
    if (!out || bytes == 0) return HS_ERR_INVALID;
    *out = nullptr;
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); *out = nullptr; return HS_ERR_HIP; }
    return HS_OK;
}
void hs_host_free(void* p) { if (p) (void)hipHostFree(p); }

// shared by hs_orb_submit_batch (grey frames: pp == nullptr, src_w x src_h IS the level-0 size) and hs_orb_submit_camera_batch (pp: the camera's own frames;
// ImageProcessing::PreProcessImg runs on the compute stream between the copy-in and the pyramid)
static int submit_frames(hs_orb* h, const uint8_t* const* imgs, int batch, int src_w, int src_h, size_t stride, const hs_preprocess_params* pp, const hs_stereo_params* sp, int32_t* ticket)
{
    for (int i = 0; i < batch; i++) if (!imgs[i]) return hs_fail(h, HS_ERR_INVALID, "null image in batch");
    FramePlan u;
    int rc = plan_frames(h, src_w, src_h, pp, &u);
    if (rc != HS_OK) return rc;
    *ticket = 0;
    h->pub_kps = nullptr; h->pub_desc = nullptr; h->pub_batch = 0;      // a slot's device block may be rewritten from here on
    HIP_TRY(h, hipSetDevice(h->device));
    hs_orb::IngestSlot* sl = nullptr;
    for (auto& c : h->slot) if (!c.busy) { sl = &c; break; }
    if (!sl) return hs_fail(h, HS_ERR_INVALID, "both staging slots are in flight: hs_orb_wait for the oldest ticket first");
    if (!h->s_in) {
        HIP_TRY(h, hipStreamCreateWithFlags(&h->s_in, hipStreamNonBlocking));
        HIP_TRY(h, hipStreamCreateWithFlags(&h->s_out, hipStreamNonBlocking));
    }
    if (!sl->ev_in) {
        HIP_TRY(h, hipEventCreateWithFlags(&sl->ev_in, hipEventDisableTiming));
        HIP_TRY(h, hipEventCreateWithFlags(&sl->ev_done, hipEventDisableTiming));
        HIP_TRY(h, hipEventCreateWithFlags(&sl->ev_out, hipEventDisableTiming));
    }
    if (!(u.gw == h->geo.w && u.gh == h->geo.h && batch <= h->geo.batch_cap)) {      // a new geometry rebuilds the shared workspace: nothing may be in flight on it
        HIP_TRY(h, hipStreamSynchronize(h->s_in)); HIP_TRY(h, hipStreamSynchronize(h->s_out));
    }
    rc = configure(h, u.gw, u.gh, batch);
    if (rc != HS_OK) return rc;
    const int cap = h->geo.max_kp, pairs = sp ? batch / 2 : 0;
    if (cap < 1) return hs_fail(h, HS_ERR_INVALID, "this frame size yields no keypoints");
    const OutLayout o = out_layout(batch, cap, pairs);
    HIP_TRY(h, sl->d_out.grow(o.bytes));             // the slot is idle: its last batch was waited for
    HIP_TRY(h, sl->h_out.grow(o.bytes));
    if (sp) {
        HIP_TRY(h, h->st.grow((size_t)pairs * cap, h->stream));
        rc = ensure_stereo_strips(h, pairs, cap, sp->n_rows);
        if (rc != HS_OK) return rc;
    }
    // From here on work is ENQUEUED that targets the slot's buffers: whatever fails below, the three streams are drained before the call returns,
    // so that a slot handed out again (it stays !busy) is never written by a copy or a kernel of the failed attempt.
    auto enqueue = [&]() -> int {
    // copy-in stream: the compute stream keeps running the previous batch meanwhile
    rc = upload_frames(h, sl->in, nullptr, u, pp != nullptr, imgs, batch, stride, false, h->s_in);
    if (rc != HS_OK) return rc;
    HIP_TRY(h, hipEventRecord(sl->ev_in, h->s_in));
    hipStream_t s = h->stream;
    HIP_TRY(h, hipStreamWaitEvent(s, sl->ev_in, 0));
    if (pp) { rc = preprocess_frames(h, sl->in, u, *pp, batch, s); if (rc != HS_OK) return rc; }
    int32_t* d_n = reinterpret_cast<int32_t*>(sl->d_out.p);
    hs_keypoint* d_k = reinterpret_cast<hs_keypoint*>(sl->d_out + o.off_k);
    uint8_t* d_d = sl->d_out + o.off_d;
    const uint8_t* const d_in = sl->in.d_in;
    if (sp) {      // images [0, pairs) are the left frames, [pairs, 2 pairs) the right ones (hs_stereo_frontend_batch_device's layout)
        HsImg0 img0{ d_in, d_in + u.per_img * pairs, pairs, (uint64_t)u.pitch, (uint64_t)u.per_img };
        HsOut out{ d_k, d_d, d_n, d_k + (size_t)pairs * cap, d_d + (size_t)pairs * cap * HS_DESC_BYTES, d_n + pairs, pairs, cap };
        rc = run_stereo_frontend(h, img0, out, *sp, reinterpret_cast<float*>(sl->d_out + o.off_u), reinterpret_cast<float*>(sl->d_out + o.off_z), s);
    } else {
        HsImg0 img0{ d_in, d_in, batch, (uint64_t)u.pitch, (uint64_t)u.per_img };
        HsOut out{ d_k, d_d, d_n, d_k, d_d, d_n, batch, cap };
        rc = run_extract(h, img0, batch, out, s);
    }
    if (rc != HS_OK) return rc;
    HIP_TRY(h, hipEventRecord(sl->ev_done, s));
    HIP_TRY(h, hipStreamWaitEvent(h->s_out, sl->ev_done, 0));
    HIP_TRY(h, hipMemcpyAsync(sl->h_out, sl->d_out, o.bytes, hipMemcpyDeviceToHost, h->s_out));
    HIP_TRY(h, hipEventRecord(sl->ev_out, h->s_out));
    return HS_OK;
    };
    rc = enqueue();
    if (rc != HS_OK) {
        const std::string why = h->err;
        (void)hipStreamSynchronize(h->s_in); (void)hipStreamSynchronize(h->stream); (void)hipStreamSynchronize(h->s_out); (void)hipGetLastError();
        h->err = why;
        return rc;
    }
    sl->busy = true; sl->batch = batch; sl->pairs = pairs; sl->cap = cap;
    sl->ticket = h->next_ticket++;
    if (h->next_ticket <= 0) h->next_ticket = 1;
    *ticket = sl->ticket;
    return HS_OK;
}

int hs_orb_submit_batch(hs_orb* h, const uint8_t* const* imgs, int batch, int w, int h_px, int stride, const hs_stereo_params* sp, int32_t* ticket)
{
    if (!h) return HS_ERR_INVALID;
    if (!imgs || !ticket || batch < 1 || batch > 65535 || w < 1 || h_px < 1 || stride < w || (sp && (batch & 1))) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    return submit_frames(h, imgs, batch, w, h_px, (size_t)stride, nullptr, sp, ticket);
}

int hs_orb_submit_camera_batch(hs_orb* h, const uint8_t* const* imgs, int batch, int w, int h_px, size_t row_stride, const hs_preprocess_params* pp,
                               const hs_stereo_params* sp, int32_t* ticket)
{
    if (!h) return HS_ERR_INVALID;
    if (!preprocess_params_ok(pp) || !imgs || !ticket || batch < 1 || batch > 65535 || w < 1 || h_px < 1 || w > 32768 || h_px > 32768 ||
        row_stride < (size_t)w * pp->channels || (sp && (batch & 1)))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    return submit_frames(h, imgs, batch, w, h_px, row_stride, pp, sp, ticket);
}

int hs_orb_wait(hs_orb* h, int32_t ticket, hs_keypoint* kps, uint8_t* desc, int32_t* n, int cap, float* uRight, float* depth)
{
    if (!h) return HS_ERR_INVALID;
    hs_orb::IngestSlot* sl = nullptr;
    for (auto& c : h->slot) if (c.busy && c.ticket == ticket) sl = &c;
    if (!sl || ticket <= 0) return hs_fail(h, HS_ERR_INVALID, "unknown ticket");
    if (!kps || !desc || !n || (sl->pairs && (!uRight || !depth))) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (cap < sl->cap) return hs_fail(h, HS_ERR_CAPACITY, "cap < keypoints this frame size can produce; see hs_orb_max_keypoints");
    HIP_TRY(h, hipSetDevice(h->device));
    {
        const hipError_t e = hipEventSynchronize(sl->ev_out);
        if (e != hipSuccess) {      // the results will never arrive: drain what can be drained and give the slot back (a ticket that fails must not block its slot for ever)
            (void)hipGetLastError();
            (void)hipStreamSynchronize(h->s_in); (void)hipStreamSynchronize(h->stream); (void)hipStreamSynchronize(h->s_out); (void)hipGetLastError();
            sl->busy = false;
            return hs_fail(h, HS_ERR_HIP, std::string("hipEventSynchronize(ticket): ") + hipGetErrorString(e));
        }
    }
    const OutLayout o = out_layout(sl->batch, sl->cap, sl->pairs);
    scatter_results(sl->h_out, o, sl->batch, sl->cap, sl->pairs, kps, desc, n, cap, uRight, depth);
    sl->busy = false;
    // (the slot's device block stays as it is until the slot is handed to another hs_orb_submit_batch)
    h->pub_kps = reinterpret_cast<const hs_keypoint*>(sl->d_out + o.off_k); h->pub_desc = sl->d_out + o.off_d; h->pub_cap = sl->cap; h->pub_batch = sl->batch;
    return HS_OK;
}

int hs_orb_cancel(hs_orb* h, int32_t ticket)
{
    if (!h) return HS_ERR_INVALID;
    hs_orb::IngestSlot* sl = nullptr;
    for (auto& c : h->slot) if (c.busy && c.ticket == ticket) sl = &c;
    if (!sl || ticket <= 0) return hs_fail(h, HS_ERR_INVALID, "unknown ticket");
    (void)hipSetDevice(h->device);
    if (hipEventSynchronize(sl->ev_out) != hipSuccess) {      // let the batch finish (its frames may be read until then), then drop the results
        (void)hipGetLastError();
        (void)hipStreamSynchronize(h->s_in); (void)hipStreamSynchronize(h->stream); (void)hipStreamSynchronize(h->s_out); (void)hipGetLastError();
    }
    sl->busy = false;
    return HS_OK;
}

int hs_ticket_frames_copied(hs_orb* h, int32_t ticket)
{
    if (!h) return HS_ERR_INVALID;
    for (auto& c : h->slot) if (c.busy && c.ticket == ticket) { const hipError_t e = hipEventQuery(c.ev_in); (void)hipGetLastError(); return e == hipSuccess ? 1 : 0; }
    return -1;
}

// ================= device-resident frames (FeatureViews stay in HBM between ImageProcessing and Tracking) =================
// hySLAM copies a frame's keypoints and descriptors out of the extractor into FeatureViews (host objects), and every matcher call gathers them
// again and uploads them (Frame.cc:45-72, FeatureViews.h:20-81).  The features were produced on this device a moment earlier: hs_frame_publish
// keeps a copy of one extracted frame in a small per-device cache (device-to-device, on the extractor's stream), hs_frame_find recognises a frame by
// its keypoint array (exact comparison with the host copy kept beside the slot — hySLAM has no field that could carry a token through FeatureViews),
// and the *_frame(s) entry points take the keypoints and descriptors from the cache instead of the host.  A slot is reused oldest first; a token
// whose slot was reused is simply unknown again (HS_ERR_INVALID) and the caller falls back to the host-pointer call.
namespace {
constexpr int HS_FRAME_SLOTS = 16;
struct FrameSlot {
    uint64_t token = 0, stamp = 0;     // token 0 = empty
    int n = 0, readers = 0;
    HsBuf<hs_keypoint> d_kps; HsBuf<uint8_t> d_desc;   // regrown behind `ready`; leaked with the cache at process exit (HsBuf's destructor never runs there)
    std::vector<hs_keypoint> h_kps;
    hipEvent_t ready = nullptr;        // recorded behind the copy that filled the slot
};
struct FrameCache { int device = 0; FrameSlot slot[HS_FRAME_SLOTS]; };
std::mutex g_frames_mu;
std::vector<FrameCache*> g_frames;     // one per device that ever published; never freed (process lifetime: static destructors must not call HIP)
uint64_t g_frame_serial = 0;
FrameCache* frame_cache_of(int device, bool create)
{
    for (FrameCache* c : g_frames) if (c->device == device) return c;
    if (!create) return nullptr;
    FrameCache* c = new FrameCache(); c->device = device; g_frames.push_back(c);
    return c;
}
struct FrameRef { FrameSlot* slot = nullptr; const hs_keypoint* d_kps = nullptr; const uint8_t* d_desc = nullptr; int n = 0; hipEvent_t ready = nullptr; };
bool frame_acquire(hs_frame_token tok, int device, FrameRef* r)
{
    std::lock_guard<std::mutex> g(g_frames_mu);
    FrameCache* c = frame_cache_of(device, false);
    if (!c || !tok) return false;
    for (FrameSlot& sl : c->slot) if (sl.token == tok) { sl.readers++; r->slot = &sl; r->d_kps = sl.d_kps; r->d_desc = sl.d_desc; r->n = sl.n; r->ready = sl.ready; return true; }
    return false;
}
void frame_release(FrameRef* r) { if (r->slot) { std::lock_guard<std::mutex> g(g_frames_mu); r->slot->readers--; r->slot = nullptr; } }
struct FrameGuard { FrameRef* a; FrameRef* b; ~FrameGuard() { if (a) frame_release(a); if (b) frame_release(b); } };
}

int hs_frame_publish(hs_orb* h, int image, const hs_keypoint* kps, int n, hs_frame_token* token)
{
    if (!h) return HS_ERR_INVALID;
    if (token) *token = 0;
    if (!token || !kps || n < 1 || n > 65535 || image < 0) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (!h->pub_kps || image >= h->pub_batch || n > h->pub_cap) return hs_fail(h, HS_ERR_INVALID, "hs_frame_publish: no host-pointer extraction result of this handle to publish (call right after hs_orb_extract / hs_orb_extract_batch / hs_orb_wait)");
    HIP_TRY(h, hipSetDevice(h->device));
    // The slot is picked and RESERVED under the process-wide lock (readers = -1: neither a publisher nor a reader nor hs_frame_cache_clear touches it),
    // the HIP calls (event wait, a possible free + allocation, two copy enqueues) run without it — hs_frame_find / frame_acquire / hs_frame_release of other
    // threads (the tracking thread's SearchByProjection) never wait behind an extractor thread's allocation — and the slot is published under the lock again.
    FrameSlot* sl = nullptr;
    {
        std::lock_guard<std::mutex> g(g_frames_mu);
        FrameCache* c = frame_cache_of(h->device, true);
        for (FrameSlot& q : c->slot) if (q.readers == 0 && (!sl || (q.token == 0 && sl->token != 0) || ((q.token == 0) == (sl->token == 0) && q.stamp < sl->stamp))) sl = &q;
        if (!sl) return hs_fail(h, HS_ERR_CAPACITY, "hs_frame_publish: every cache slot is being read");
        sl->token = 0;
        sl->readers = -1;
    }
    struct Unreserve { FrameSlot* s; ~Unreserve() { if (s) { std::lock_guard<std::mutex> g(g_frames_mu); s->readers = 0; } } } unreserve{sl};      // failure paths: the slot is empty (token 0) and free again
    if (!sl->ready) HIP_TRY(h, hipEventCreateWithFlags(&sl->ready, hipEventDisableTiming));
    if ((size_t)n > sl->d_kps.cap) {
        HIP_TRY(h, hipEventSynchronize(sl->ready));      // (a never-recorded event is complete)
        const size_t room = (size_t)std::max(n, 2048);
        HIP_TRY(h, sl->d_kps.grow(room));
        HIP_TRY(h, sl->d_desc.grow(room * HS_DESC_BYTES));
    }
    hipStream_t s = h->stream;
    HIP_TRY(h, hipStreamWaitEvent(s, sl->ready, 0));     // the copy that filled the slot last time (another handle's stream) comes first
    HIP_TRY(h, hipMemcpyAsync(sl->d_kps, h->pub_kps + (size_t)image * h->pub_cap, (size_t)n * sizeof(hs_keypoint), hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(sl->d_desc, h->pub_desc + (size_t)image * h->pub_cap * HS_DESC_BYTES, (size_t)n * HS_DESC_BYTES, hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipEventRecord(sl->ready, s));
    sl->h_kps.assign(kps, kps + n);                      // (the slot is reserved: nobody compares against h_kps while token == 0)
    {
        std::lock_guard<std::mutex> g(g_frames_mu);
        unreserve.s = nullptr;
        sl->readers = 0;
        sl->n = n; sl->stamp = ++g_frame_serial; sl->token = sl->stamp;
        *token = sl->token;
    }
    return HS_OK;
}

int hs_frame_find(int device, const hs_keypoint* kps, int n, hs_frame_token* token)
{
    if (!token) return HS_ERR_INVALID;
    *token = 0;
    if (!kps || n < 1) return HS_ERR_INVALID;
    std::lock_guard<std::mutex> g(g_frames_mu);
    FrameCache* c = frame_cache_of(device, false);
    if (!c) return HS_ERR_INVALID;
    const FrameSlot* best = nullptr;
    for (const FrameSlot& sl : c->slot)
        if (sl.token && sl.n == n && (!best || sl.stamp > best->stamp) && memcmp(sl.h_kps.data(), kps, (size_t)n * sizeof(hs_keypoint)) == 0) best = &sl;
    if (!best) return HS_ERR_INVALID;
    *token = best->token;
    return HS_OK;
}

int hs_frame_release(int device, hs_frame_token token)
{
    std::lock_guard<std::mutex> g(g_frames_mu);
    FrameCache* c = frame_cache_of(device, false);
    if (!c || !token) return HS_ERR_INVALID;
    for (FrameSlot& sl : c->slot) if (sl.token == token) { sl.token = 0; return HS_OK; }      // (a slot that is being read keeps its buffers until the reader is done: readers > 0 keeps it from being refilled)
    return HS_ERR_INVALID;
}

int hs_frame_cache_clear(int device)
{
    std::lock_guard<std::mutex> g(g_frames_mu);
    for (size_t i = 0; i < g_frames.size(); i++) {
        FrameCache* c = g_frames[i];
        if (c->device != device) continue;
        for (const FrameSlot& sl : c->slot) if (sl.readers != 0) return HS_ERR_INVALID;      // a call is reading a slot (> 0) or a publisher is filling one (-1): not now
        int cur = -1;
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(device);
        for (FrameSlot& sl : c->slot) {
            if (sl.ready) { (void)hipEventSynchronize(sl.ready); (void)hipEventDestroy(sl.ready); }
            sl.d_kps.release(); sl.d_desc.release();
        }
        if (cur >= 0) (void)hipSetDevice(cur);
        delete c;
        g_frames.erase(g_frames.begin() + (long)i);
        return HS_OK;
    }
    return HS_OK;      // nothing was ever published on that device
}

int hs_frame_info(int device, hs_frame_token token, int32_t* n)
{
    std::lock_guard<std::mutex> g(g_frames_mu);
    FrameCache* c = frame_cache_of(device, false);
    if (!c || !token) return HS_ERR_INVALID;
    for (const FrameSlot& sl : c->slot) if (sl.token == token) { if (n) *n = sl.n; return HS_OK; }
    return HS_ERR_INVALID;
}

// what hs_search_by_projection and hs_search_by_projection_frame do once their arguments are checked and L > 0.  ref: the published frame that
// supplies keypoints and descriptors (the launches wait for it), nullptr: they are staged from F
static int search_by_projection_host(hs_orb* h, const FrameRef* ref, const hs_frame_view* F, const hs_landmark* lms, int L, const hs_proj_params* pp,
                                     int32_t* match_idx, float* match_dist, int32_t* n_matches)
{
    HIP_TRY(h, hipSetDevice(h->device));
    const int n = F->n;
    HsStage st(h);
    DevFrame D{}; float *d_uR, *d_mdist, *d_pangle; int32_t *d_obs, *d_winner, *d_midx, *d_nm; hs_landmark* d_lms;
    if (ref) st.temp(&D.cell, hs_frame_grid_bytes(n)); else stage_frame(st, F, &D);
    st.in(&d_uR, n, F->uR); st.in(&d_obs, n, F->kp_lm_obs); st.temp(&d_winner, n);
    st.in(&d_lms, L, lms);
    st.out(&d_midx, L, match_idx); st.out(&d_mdist, L, match_dist); st.temp(&d_pangle, L); st.out(&d_nm, 1, n_matches);
    int rc = st.begin();
    if (rc != HS_OK) return rc;
    hipStream_t s = st.stream();
    if (ref) HIP_TRY(h, hipStreamWaitEvent(s, ref->ready, 0));
    const hs_keypoint* d_kps = ref ? ref->d_kps : D.kps;
    hs_launch_frame_grid(*F, d_kps, D.cell, true, s);
    hs_launch_search_projection(*F, d_kps, ref ? ref->d_desc : D.desc, F->uR ? d_uR : nullptr, F->kp_lm_obs ? d_obs : nullptr, D.cell, d_lms, L, *pp,
                                d_midx, d_mdist, d_winner, d_pangle, d_nm, s);
    rc = st.finish();
    if (rc != HS_OK) return rc;
    for (int i = 0; i < L; i++) if (match_idx[i] < 0) match_dist[i] = -1.f;      // entries dropped by the rotation check
    return HS_OK;
}

int hs_search_by_projection(hs_orb* h, const hs_frame_view* F, const hs_landmark* lms, int L, const hs_proj_params* pp,
                            int32_t* match_idx, float* match_dist, int32_t* n_matches)
{
    if (!h) return HS_ERR_INVALID;
    if (!F || !pp || L < 0 || !n_matches || (L > 0 && (!lms || !match_idx || !match_dist)) || F->n < 0 || F->n > 65535 ||
        (F->n > 0 && (!F->kps || !F->desc)) || (pp->use_stereo && F->sensor != 0 && F->n > 0 && !F->uR))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    *n_matches = 0;
    if (L == 0) return HS_OK;
    return search_by_projection_host(h, nullptr, F, lms, L, pp, match_idx, match_dist, n_matches);
}

int hs_search_by_projection_frame(hs_orb* h, hs_frame_token frame, const hs_frame_view* F, const hs_landmark* lms, int L, const hs_proj_params* pp,
                                  int32_t* match_idx, float* match_dist, int32_t* n_matches)
{
    if (!h) return HS_ERR_INVALID;
    if (!F || !pp || L < 0 || !n_matches || (L > 0 && (!lms || !match_idx || !match_dist)) || F->n < 1 || F->n > 65535 ||
        (pp->use_stereo && F->sensor != 0 && !F->uR))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    *n_matches = 0;
    FrameRef ref;
    if (!frame_acquire(frame, h->device, &ref)) return hs_fail(h, HS_ERR_INVALID, "hs_search_by_projection_frame: unknown frame token (its cache slot was reused, or it lives on another device)");
    FrameGuard guard{ &ref, nullptr };
    if (ref.n != F->n) return hs_fail(h, HS_ERR_INVALID, "hs_search_by_projection_frame: F->n differs from the published frame");
    if (L == 0) return HS_OK;
    return search_by_projection_host(h, &ref, F, lms, L, pp, match_idx, match_dist, n_matches);
}

int hs_stereo_match_frames(hs_orb* h, hs_frame_token left, hs_frame_token right, const hs_stereo_params* sp, float* uRight, float* depth)
{
    if (!h) return HS_ERR_INVALID;
    if (!sp || !uRight || !depth) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    FrameRef L, R;
    if (!frame_acquire(left, h->device, &L)) return hs_fail(h, HS_ERR_INVALID, "hs_stereo_match_frames: unknown left frame token");
    FrameGuard guard{ &L, nullptr };
    if (!frame_acquire(right, h->device, &R)) return hs_fail(h, HS_ERR_INVALID, "hs_stereo_match_frames: unknown right frame token");
    guard.b = &R;
    HIP_TRY(h, hipSetDevice(h->device));
    const int nL = L.n, nR = R.n, cap = std::max(nL, nR);
    const int rc = stereo_pair_buffers(h, 0, cap, sp->n_rows);
    if (rc != HS_OK) return rc;
    return stereo_pair_tail(h, 0, nL, nR, L.d_kps, L.d_desc, R.d_kps, R.d_desc, cap, *sp, L.ready, R.ready, uRight, depth);
}

int hs_frame_grid(hs_orb* h, const hs_frame_view* F, int8_t* cell_xy)
{
    if (!h) return HS_ERR_INVALID;
    if (!F || F->n < 0 || F->n > 65535 || (F->n > 0 && (!F->kps || !cell_xy))) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (F->n == 0) return HS_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HsStage st(h);
    hs_keypoint* d_kps; int8_t* d_cell;
    st.in(&d_kps, F->n, F->kps); st.out(&d_cell, hs_frame_grid_bytes(F->n), cell_xy, (size_t)F->n * 2);
    int rc = st.begin();
    if (rc != HS_OK) return rc;
    hs_launch_frame_grid(*F, d_kps, d_cell, false, st.stream());
    return st.finish();
}

} // extern "C"
int hs_search_by_projection_enqueue(hs_orb* h, const hs_frame_view* F, const hs_pose_view* d_pose, const hs_landmark* d_lms, int L, const hs_proj_params* pp,
                                    int32_t* d_match_idx, float* d_match_dist, int32_t* d_n_matches, hipStream_t s)
{
    // temporaries only, and no synchronisation: the call runs on the caller's stream.  Scratch is per handle: a second call may only start
    // after the first finished (same stream ordering is enough)
    HsStage st(h, s);                                            // (under hs_debug_poison the fill is ordered in front of the launches)
    int8_t* d_cell; int32_t* d_winner; float* d_pangle;
    st.temp(&d_cell, hs_frame_grid_bytes(F->n)); st.temp(&d_winner, F->n); st.temp(&d_pangle, L);
    const int rc = st.begin();
    if (rc != HS_OK) return rc;
    hs_launch_frame_grid(*F, F->kps, d_cell, true, s);
    hs_launch_search_projection(*F, F->kps, F->desc, F->uR, F->kp_lm_obs, d_cell, d_lms, L, *pp, d_match_idx, d_match_dist, d_winner, d_pangle, d_n_matches, s, d_pose);
    return HS_OK;
}
extern "C" {
int hs_search_by_projection_device(hs_orb* h, const hs_frame_view* F, const hs_landmark* d_lms, int L, const hs_proj_params* pp,
                                   int32_t* d_match_idx, float* d_match_dist, int32_t* d_n_matches, void* stream)
{
    return hs_device_call(h, hs_search_by_projection_why(F, d_lms, L, pp, d_match_idx, d_match_dist, d_n_matches), stream,
                          [&](hipStream_t s) { return hs_search_by_projection_enqueue(h, F, nullptr, d_lms, L, pp, d_match_idx, d_match_dist, d_n_matches, s); });
}
// the pose from device memory (hs_pose_views_device): F's Rcw / tcw / Ow are not read
int hs_search_by_projection_posed_device(hs_orb* h, const hs_frame_view* F, const hs_pose_view* d_pose, const hs_landmark* d_lms, int L, const hs_proj_params* pp,
                                         int32_t* d_match_idx, float* d_match_dist, int32_t* d_n_matches, void* stream)
{
    return hs_device_call(h, d_pose ? hs_search_by_projection_why(F, d_lms, L, pp, d_match_idx, d_match_dist, d_n_matches) : "bad argument", stream,
                          [&](hipStream_t s) { return hs_search_by_projection_enqueue(h, F, d_pose, d_lms, L, pp, d_match_idx, d_match_dist, d_n_matches, s); });
}

namespace {
// one row of A*B (+c): double accumulation, alpha in double, one rounding (cv::gemm on float matrices)
float gemm3h(const float* A, const float* B, float c, double alpha = 1.0)
{
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)A[k] * (double)B[k];
    return (float)(alpha * s + (double)c);
}
}

int hs_search_by_projection_sim3(hs_orb* h, const hs_frame_view* KF, const float* Scw, const hs_landmark* lms, int L, int th, float th_low,
                                 uint8_t* kp_matched, int32_t* match_idx, int32_t* n_matches)
{
    if (!h) return HS_ERR_INVALID;
    if (!KF || !Scw || L < 0 || !n_matches || (L > 0 && (!lms || !match_idx)) || KF->n < 0 || KF->n > 65535 || (KF->n > 0 && (!KF->kps || !KF->desc || !kp_matched)))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    *n_matches = 0;
    for (int i = 0; i < L; i++) match_idx[i] = -1;
    if (L == 0 || KF->n == 0) return HS_OK;
    // Decompose Scw like the reference (FeatureMatcher.cc:641-646): scw = |row 0| (double accumulation), Rcw = sRcw/scw and tcw = t/scw are
    // cv::Mat scalings (every element times (float)(1/scw) in float), Ow = -Rcw.t()*tcw one gemm
    float R[9], t[3], Ow[3];
    const float scw = (float)std::sqrt((double)Scw[0] * Scw[0] + (double)Scw[1] * Scw[1] + (double)Scw[2] * Scw[2]);
    const float inv = (float)(1.0 / (double)scw);
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) R[3 * r + c] = Scw[4 * r + c] * inv + 0.0f; t[r] = Scw[4 * r + 3] * inv + 0.0f; }
    for (int i = 0; i < 3; i++) { const float col[3] = { R[i], R[3 + i], R[6 + i] }; Ow[i] = gemm3h(col, t, 0.f, -1.0); }
    HIP_TRY(h, hipSetDevice(h->device));
    HsStage st(h);
    DevFrame D; hs_landmark* d_lms; float* d_geo; uint8_t* d_taken; int32_t *d_midx, *d_n;
    stage_frame(st, KF, &D);
    st.in(&d_lms, L, lms); st.temp(&d_geo, (size_t)L * 3);
    st.inout(&d_taken, KF->n, kp_matched); st.out(&d_midx, L, match_idx); st.out(&d_n, 1, n_matches);
    int rc = st.begin();
    if (rc != HS_OK) return rc;
    hs_launch_frame_grid(*KF, D.kps, D.cell, true, st.stream());
    hs_launch_sim3_projection(*KF, D.kps, D.desc, D.cell, R, t, Ow, d_lms, L, (float)th, th_low, d_geo, d_taken, d_midx, d_n, st.stream());
    return st.finish();
}

int hs_search_by_sim3(hs_orb* h, const hs_frame_view* KF1, const hs_landmark* lms1, const hs_frame_view* KF2, const hs_landmark* lms2,
                      float s12, const float* R12, const float* t12, float th, float th_high, int32_t* match12, int32_t* n_found)
{
    if (!h) return HS_ERR_INVALID;
    if (!KF1 || !KF2 || !R12 || !t12 || !n_found || KF1->n < 0 || KF2->n < 0 || KF1->n > 65535 || KF2->n > 65535 ||
        (KF1->n > 0 && (!KF1->kps || !KF1->desc || !lms1 || !match12)) || (KF2->n > 0 && (!KF2->kps || !KF2->desc || !lms2)))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    *n_found = 0;
    for (int i = 0; i < KF1->n; i++) match12[i] = -1;
    if (KF1->n == 0 || KF2->n == 0) return HS_OK;
    // Transformation between cameras (FeatureMatcher.cc:757-760): sR12 = s12*R12, sR21 = (1/s12)*R12.t() (cv::Mat scalings), t21 = -sR21*t12 (gemm)
    float sR12[9], sR21[9], t21[3];
    const float a12 = (float)(double)s12, a21 = (float)(1.0 / (double)s12);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { sR12[3 * r + c] = R12[3 * r + c] * a12 + 0.0f; sR21[3 * r + c] = R12[3 * c + r] * a21 + 0.0f; }
    for (int i = 0; i < 3; i++) t21[i] = gemm3h(&sR21[3 * i], t12, 0.f, -1.0);
    HIP_TRY(h, hipSetDevice(h->device));
    const int n1 = KF1->n, n2 = KF2->n;
    HsStage st(h);
    DevFrame D1, D2; hs_landmark *d_l1, *d_l2; int32_t *d_m1, *d_m12, *d_m2, *d_n;
    stage_frame(st, KF1, &D1); stage_frame(st, KF2, &D2);
    st.in(&d_l1, n1, lms1); st.in(&d_l2, n2, lms2);
    st.temp(&d_m1, n1); st.out(&d_m12, n1, match12); st.temp(&d_m2, n2); st.out(&d_n, 1, n_found);
    int rc = st.begin();
    if (rc != HS_OK) return rc;
    hipStream_t s = st.stream();
    hs_launch_frame_grid(*KF1, D1.kps, D1.cell, true, s);
    hs_launch_frame_grid(*KF2, D2.kps, D2.cell, true, s);
    hs_launch_sim3_search(*KF1, D1.kps, D1.desc, D1.cell, *KF2, D2.kps, D2.desc, D2.cell, d_l1, d_l2, sR21, t21, sR12, t12, th, th_high, d_m1, d_m2, d_m12, d_n, s);
    return st.finish();
}

int hs_search_by_bow(hs_orb* h, const hs_keypoint* kps1, const uint8_t* desc1, int n1,
                     const int32_t* node_id1, const int32_t* node_ptr1, const int32_t* idx1, int nn1,
                     const hs_keypoint* kps2, const uint8_t* desc2, int n2,
                     const int32_t* node_id2, const int32_t* node_ptr2, const int32_t* idx2, int nn2,
                     const uint8_t* keep1, float score_threshold, float second_best_ratio, int check_rotation,
                     int32_t* match12, int32_t* n_matches)
{
    return hs_search_by_bow_ex(h, kps1, desc1, n1, node_id1, node_ptr1, idx1, nn1, kps2, desc2, n2, node_id2, node_ptr2, idx2, nn2,
                               keep1, nullptr, nullptr, 31.f, 1.f, score_threshold, second_best_ratio, check_rotation, match12, n_matches);
}

static int bow_host(hs_orb* h, int legacy, const hs_keypoint* kps1, const uint8_t* desc1, int n1,
                        const int32_t* node_id1, const int32_t* node_ptr1, const int32_t* idx1, int nn1,
                        const hs_keypoint* kps2, const uint8_t* desc2, int n2,
                        const int32_t* node_id2, const int32_t* node_ptr2, const int32_t* idx2, int nn2,
                        const uint8_t* keep1, const uint8_t* keep2, const float* F12, float size_ref, float sigma_ref,
                        float score_threshold, float second_best_ratio, int check_rotation,
                        int32_t* match12, int32_t* n_matches)
{
    if (!h) return HS_ERR_INVALID;
    if (n1 < 0 || n2 < 0 || nn1 < 0 || nn2 < 0 || !n_matches || (n1 > 0 && (!kps1 || !desc1 || !match12)) || (n2 > 0 && (!kps2 || !desc2)) ||
        (nn1 > 0 && (!node_id1 || !node_ptr1 || !idx1)) || (nn2 > 0 && (!node_id2 || !node_ptr2 || !idx2)))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    for (int a = 0; a < nn1; a++) if (node_ptr1[a] < 0 || node_ptr1[a + 1] < node_ptr1[a]) return hs_fail(h, HS_ERR_INVALID, "feature vector node_ptr must be non-negative and non-decreasing");
    for (int b = 0; b < nn2; b++) if (node_ptr2[b] < 0 || node_ptr2[b + 1] < node_ptr2[b]) return hs_fail(h, HS_ERR_INVALID, "feature vector node_ptr must be non-negative and non-decreasing");
    *n_matches = 0;
    for (int i = 0; i < n1; i++) match12[i] = -1;
    if (n1 == 0 || n2 == 0 || nn1 == 0 || nn2 == 0) return HS_OK;
    // merge-walk of the two DBoW2::FeatureVector maps (FeatureMatcher.cc:230-265): nodes present on both sides
    std::vector<int32_t> pa, pb;
    for (int a = 0, b = 0; a < nn1 && b < nn2;) {
        if (node_id1[a] == node_id2[b]) { pa.push_back(a++); pb.push_back(b++); }
        else if (node_id1[a] < node_id2[b]) a++; else b++;
    }
    const int np = (int)pa.size();
    const int m1 = node_ptr1[nn1], m2 = node_ptr2[nn2];
    for (int i = 0; i < m1; i++) if (idx1[i] < 0 || idx1[i] >= n1) return hs_fail(h, HS_ERR_INVALID, "feature vector index out of range");
    for (int i = 0; i < m2; i++) if (idx2[i] < 0 || idx2[i] >= n2) return hs_fail(h, HS_ERR_INVALID, "feature vector index out of range");
    HIP_TRY(h, hipSetDevice(h->device));
    HsStage st(h);
    hs_keypoint *d_k1, *d_k2; uint8_t *d_d1, *d_d2, *d_keep, *d_keep2; int32_t *d_p1, *d_p2, *d_i1, *d_i2, *d_pa, *d_pb, *d_m, *d_self, *d_nm;
    float* d_ang; uint32_t* d_taken2;
    st.in(&d_k1, n1, kps1); st.in(&d_k2, n2, kps2); st.in(&d_d1, (size_t)n1 * 32, desc1); st.in(&d_d2, (size_t)n2 * 32, desc2);
    st.in(&d_p1, nn1 + 1, node_ptr1); st.in(&d_p2, nn2 + 1, node_ptr2); st.in(&d_i1, m1, idx1); st.in(&d_i2, m2, idx2);
    st.in(&d_pa, np, pa.data()); st.in(&d_pb, np, pb.data());
    st.in(&d_keep, n1, keep1); st.in(&d_keep2, n2, keep2);
    st.out(&d_m, n1, match12); st.temp(&d_ang, n1); st.temp(&d_self, n1); st.out(&d_nm, 1, n_matches); st.temp(&d_taken2, n2);
    int rc = st.begin();
    if (rc != HS_OK) return rc;
    hipStream_t s = st.stream();
    if (legacy)
        hs_launch_bow_legacy(d_pa, d_pb, np, d_p1, d_i1, d_p2, d_i2, d_d1, d_d2, keep1 ? d_keep : nullptr, keep2 ? d_keep2 : nullptr,
                             score_threshold, second_best_ratio, d_m, n1, n2, d_k1, d_k2, d_ang, check_rotation, d_self, d_taken2, d_nm, s);
    else
        hs_launch_bow(d_pa, d_pb, np, d_p1, d_i1, d_p2, d_i2, d_d1, d_d2, keep1 ? d_keep : nullptr, keep2 ? d_keep2 : nullptr,
                      F12, size_ref, sigma_ref, score_threshold, second_best_ratio,
                      d_m, n1, d_k1, d_k2, d_ang, check_rotation, d_self, d_nm, s);
    return st.finish();
}

int hs_search_by_bow_ex(hs_orb* h, const hs_keypoint* kps1, const uint8_t* desc1, int n1,
                        const int32_t* node_id1, const int32_t* node_ptr1, const int32_t* idx1, int nn1,
                        const hs_keypoint* kps2, const uint8_t* desc2, int n2,
                        const int32_t* node_id2, const int32_t* node_ptr2, const int32_t* idx2, int nn2,
                        const uint8_t* keep1, const uint8_t* keep2, const float* F12, float size_ref, float sigma_ref,
                        float score_threshold, float second_best_ratio, int check_rotation,
                        int32_t* match12, int32_t* n_matches)
{
    return bow_host(h, 0, kps1, desc1, n1, node_id1, node_ptr1, idx1, nn1, kps2, desc2, n2, node_id2, node_ptr2, idx2, nn2, keep1, keep2, F12, size_ref, sigma_ref,
                    score_threshold, second_best_ratio, check_rotation, match12, n_matches);
}

int hs_search_by_bow_legacy(hs_orb* h, const hs_keypoint* kps1, const uint8_t* desc1, int n1,
                            const int32_t* node_id1, const int32_t* node_ptr1, const int32_t* idx1, int nn1,
                            const hs_keypoint* kps2, const uint8_t* desc2, int n2,
                            const int32_t* node_id2, const int32_t* node_ptr2, const int32_t* idx2, int nn2,
                            const uint8_t* keep1, const uint8_t* keep2, float th_low, float nnratio, int check_orientation,
                            int32_t* match12, int32_t* n_matches)
{
    return bow_host(h, 1, kps1, desc1, n1, node_id1, node_ptr1, idx1, nn1, kps2, desc2, n2, node_id2, node_ptr2, idx2, nn2, keep1, keep2, nullptr, 31.f, 1.f,
                    th_low, nnratio, check_orientation, match12, n_matches);
}

int hs_search_for_initialization(hs_orb* h, const hs_keypoint* kps1, const uint8_t* desc1, int n1, const hs_frame_view* F2,
                                 float* prev_matched_xy, int window, float th_low, float nnratio, int32_t* matches12, int32_t* n_matches)
{
    if (!h) return HS_ERR_INVALID;
    if (!F2 || n1 < 0 || !n_matches || F2->n < 0 || F2->n > 65535 || (n1 > 0 && (!kps1 || !desc1 || !prev_matched_xy || !matches12)) ||
        (F2->n > 0 && (!F2->kps || !F2->desc)))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    *n_matches = 0;
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    if (n1 == 0 || F2->n == 0) return HS_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const int n2 = F2->n;
    std::vector<int32_t> owner(n2);
    HsStage st(h);
    hs_keypoint *d_k1, *d_k2; uint8_t *d_d1, *d_d2; int8_t* d_cell; float *d_prev, *d_ang; int32_t *d_owner, *d_odist, *d_self, *d_nm;
    st.in(&d_k1, n1, kps1); st.in(&d_k2, n2, F2->kps); st.in(&d_d1, (size_t)n1 * 32, desc1); st.in(&d_d2, (size_t)n2 * 32, F2->desc);
    st.temp(&d_cell, (size_t)n2 * 2); st.in(&d_prev, (size_t)n1 * 2, prev_matched_xy);
    st.out(&d_owner, n2, owner.data()); st.temp(&d_odist, n2); st.temp(&d_ang, n2); st.temp(&d_self, n2); st.out(&d_nm, 1, n_matches);
    int rc = st.begin();
    if (rc != HS_OK) return rc;
    hs_launch_frame_grid(*F2, d_k2, d_cell, false, st.stream());
    hs_launch_search_init(*F2, d_k2, d_d2, d_cell, d_k1, d_d1, n1, d_prev, (float)window, th_low, nnratio, d_owner, d_odist, d_ang, d_self, d_nm, st.stream());
    rc = st.finish();
    if (rc != HS_OK) return rc;
    for (int i2 = 0; i2 < n2; i2++) {                          // matches_inverse + vbPrevMatched update (:446-458)
        const int i1 = owner[i2];
        if (i1 < 0) continue;
        matches12[i1] = i2;
        prev_matched_xy[2 * i1] = F2->kps[i2].x; prev_matched_xy[2 * i1 + 1] = F2->kps[i2].y;
    }
    return HS_OK;
}

int hs_bow_transform(hs_orb* h, const hs_vocab_tree* T, const uint8_t* desc, int n, int levelsup, int32_t* word_id, float* weight, int32_t* node_id)
{
    if (!h) return HS_ERR_INVALID;
    if (!T || n < 0 || T->n_nodes < 2 || T->levels < 1 || !T->child_begin || !T->child_count || !T->desc || !T->word_id || !T->weight ||
        (n > 0 && (!desc || !word_id || !weight || !node_id)))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (n == 0) return HS_OK;
    // the walk must terminate inside the tree: children in range, the root has children
    if (T->child_count[0] < 1) return hs_fail(h, HS_ERR_INVALID, "vocabulary root has no children");
    for (int i = 0; i < T->n_nodes; i++) {
        const long cb = T->child_begin[i], cc = T->child_count[i];
        if (cc < 0 || (cc > 0 && (cb <= i || cb + cc > T->n_nodes))) return hs_fail(h, HS_ERR_INVALID, "vocabulary tree is not a forward-linked flat tree");
    }
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t nn = T->n_nodes;
    HsStage st(h);
    int32_t *d_cb, *d_cc, *d_w, *o_w, *o_n; float *d_wt, *o_wt; uint8_t *d_nd, *d_d;
    st.in(&d_cb, nn, T->child_begin); st.in(&d_cc, nn, T->child_count); st.in(&d_w, nn, T->word_id); st.in(&d_wt, nn, T->weight);
    st.in(&d_nd, nn * 32, T->desc); st.in(&d_d, (size_t)n * 32, desc);
    st.out(&o_w, n, word_id); st.out(&o_wt, n, weight); st.out(&o_n, n, node_id);
    int rc = st.begin();
    if (rc != HS_OK) return rc;
    hs_launch_bow_transform(n, d_d, d_cb, d_cc, d_nd, d_w, d_wt, T->levels, levelsup, o_w, o_wt, o_n, st.stream());
    rc = st.finish();
    if (rc != HS_OK) return rc;
    if (T->orig_id) for (int i = 0; i < n; i++) node_id[i] = T->orig_id[node_id[i]];      // renumbered vocabulary: report DBoW2's NodeId
    return HS_OK;
}

int hs_hamming_knn2_device(hs_orb* h, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt,
                           int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_second_dist, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (nq < 0 || nt < 0 || (nq > 0 && (!d_q || !d_best_idx || !d_best_dist || !d_second_dist)) || (nt > 0 && !d_t)) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    hs_launch_knn2(d_q, nq, d_t, nt, d_best_idx, d_best_dist, d_second_dist, hs_stream_or(h, stream));
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_hamming_knn2(hs_orb* h, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* best_idx, int32_t* best_dist, int32_t* second_dist)
{
    if (!h) return HS_ERR_INVALID;
    if (nq < 0 || nt < 0 || (nq > 0 && (!q || !best_idx || !best_dist || !second_dist)) || (nt > 0 && !t)) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (nq == 0) return HS_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HsStage st(h);
    uint8_t *dq, *dt; int32_t *bi, *bd, *sd;
    st.in(&dq, (size_t)nq * 32, q); st.in(&dt, (size_t)nt * 32, t);
    st.out(&bi, nq, best_idx); st.out(&bd, nq, best_dist); st.out(&sd, nq, second_dist);
    int rc = st.begin();
    if (rc != HS_OK) return rc;
    hs_launch_knn2(dq, nq, dt, nt, bi, bd, sd, st.stream());
    return st.finish();
}

// [ count | pad to 16 | keypoints[cap] | pad to 16 | descriptors[cap][32] ]: the descriptor block starts on a 16-byte boundary whatever the parity of
// cap (24-byte keypoints), because the describe kernel writes a descriptor as two 16-byte vector stores
static size_t record_off_desc(int cap) { return ((size_t)HS_RECORD_HEADER + (size_t)std::max(cap, 0) * sizeof(hs_keypoint) + 15) & ~(size_t)15; }
size_t hs_record_bytes(int cap) { return cap < 0 ? 0 : record_off_desc(cap) + (size_t)cap * HS_DESC_BYTES; }

void hs_record_offsets(int cap, size_t* off_count, size_t* off_kps, size_t* off_desc)
{
    if (off_count) *off_count = 0;
    if (off_kps) *off_kps = HS_RECORD_HEADER;
    if (off_desc) *off_desc = record_off_desc(cap);
}

int hs_records_knn2_device(hs_orb* h, const uint8_t* d_records, size_t record_stride, int world, int rank, int cap,
                           int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_second_dist, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!d_records || world < 1 || world > 65535 || rank < 0 || rank >= world || cap < 1 || cap > 65535 || record_stride < hs_record_bytes(cap) ||
        (record_stride & 3) || ((uintptr_t)d_records & 15) || !d_best_idx || !d_best_dist || !d_second_dist)
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    size_t od; hs_record_offsets(cap, nullptr, nullptr, &od);
    hs_launch_knn2_records(d_records, record_stride, world, rank, cap, od, d_best_idx, d_best_dist, d_second_dist, hs_stream_or(h, stream));
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_debug_stream_copy(hs_orb* h, void* d_dst, const void* d_src, size_t bytes, int width, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    if (!d_dst || !d_src || (width != 4 && width != 16 && width != 64) || bytes % 16) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    hs_launch_stream_copy(d_dst, d_src, bytes, width, hs_stream_or(h, stream));
    HIP_TRY(h, hipGetLastError());
    return HS_OK;
}

int hs_debug_poison(int byte)
{
    if (byte < -1 || byte > 255) return HS_ERR_INVALID;
    g_hs_poison.store(byte, std::memory_order_relaxed);
    return HS_OK;
}

long long hs_debug_poison_violations(void) { return g_hs_poison_violations.load(std::memory_order_relaxed); }

int hs_debug_poison_selftest(hs_orb* h, int* reported)
{
    if (!h) return HS_ERR_INVALID;
    if (reported) *reported = 0;
    const int byte = hs_poison_byte();
    if (!reported || byte < 0) return hs_fail(h, HS_ERR_INVALID, "hs_debug_poison_selftest: poisoning is off (hs_debug_poison)");
    HIP_TRY(h, hipSetDevice(h->device));
    uint8_t src[64], back[64];
    memset(src, ~byte & 0xFF, sizeof src);
    HsStage st(h);
    uint8_t *d_a, *d_b;
    st.in(&d_a, sizeof src, src); st.out(&d_b, sizeof back, back);
    int rc = st.begin();
    if (rc != HS_OK) return rc;
    // 16 bytes of piece 0 to [64, 80) of its own 256-byte slot: padding, 176 bytes in front of piece 1 and 4 KiB + 432 bytes inside the claim
    hs_launch_stream_copy(d_a + sizeof src, d_a, 16, 16, st.stream());
    hs_launch_stream_copy(d_b, d_a, sizeof back, 16, st.stream());
    rc = st.finish();
    if (rc == HS_ERR_POISON) { *reported = 1; return HS_OK; }
    return rc;
}

int hs_orb_stage_launches(const hs_orb* h, int stage)
{
    // launches per stage OF THE LAST CALL on the handle (what hs_orb_profile_end's per-stage times are divided by): the pyramid's plan depends on the
    // batch (calls of <= deep_max_batch frames run the small-batch plan: one launch at 1080p instead of three), the stereo stage on the entry point.
    // Between a (re)configuration and the next call: the planned count of the CURRENT geometry's standard plan (the last call's figures go with
    // the geometry they were counted on).  Per lane: a second lane (hs_orb_set_lanes) enqueues as many launches again on its own stream.
    if (!h || stage < 0 || stage >= HS_NUM_STAGES) return 0;
    if (stage == 0) {
        if (h->geo.last_pyr_launches > 0) return h->geo.last_pyr_launches;      // counted by the launcher itself: a per-level fallback (caller-frame alignment, no big LDS) is included
        if (h->geo.lv.empty()) return std::max(h->p.nlevels - 1, 0);
        if (h->geo.last_batch > 0 && h->geo.last_batch <= h->knobs.deep_max_batch && !h->geo.pyr_deep.empty()) { int32_t o[8]; hs_debug_plan_summary(h, o); return o[1]; }
        return hs_pyramid_launch_count(h->geo.lv.data(), h->p.nlevels);
    }
    return stage == 4 ? h->last_stereo_launches : (stage == 2 ? h->last_qt_launches : 1);
}

int hs_orb_profile_begin(hs_orb* h)
{
    if (!h) return HS_ERR_INVALID;
    h->prof = true; h->ev_used = 0; h->prof_stage.clear();
    if (h->lane2) { h->lane2->prof = true; h->lane2->ev_used = 0; h->lane2->prof_stage.clear(); }
    return HS_OK;
}

int hs_orb_profile_pause(hs_orb* h)
{
    if (!h) return HS_ERR_INVALID;
    h->prof = false;
    if (h->lane2) h->lane2->prof = false;
    return HS_OK;
}

int hs_orb_profile_end(hs_orb* h, double* ms, int32_t* launches)
{
    if (!h) return HS_ERR_INVALID;
    if (!ms || !launches) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    for (int i = 0; i < HS_NUM_STAGES; i++) { ms[i] = 0; launches[i] = 0; }
    // the second lane (hs_orb_set_lanes) records its own event sequence: both are summed
    for (hs_orb* q : { h, h->lane2 }) {
        if (!q) continue;
        q->prof = false;
        if (q->ev_used) HIP_TRY(h, hipEventSynchronize(q->ev_pool[q->ev_used - 1]));
        for (size_t i = 0; i + 1 < q->ev_used; i++) {
            int st = q->prof_stage[i];
            if (st < 0 || st >= HS_NUM_STAGES) continue;
            float t = 0.f;
            HIP_TRY(h, hipEventElapsedTime(&t, q->ev_pool[i], q->ev_pool[i + 1]));
            ms[st] += t; launches[st]++;
        }
        q->ev_used = 0; q->prof_stage.clear();
    }
    return HS_OK;
}

int hs_orb_set_lanes(hs_orb* h, int lanes)
{
    if (!h) return HS_ERR_INVALID;
    if (lanes < 1 || lanes > 2) return hs_fail(h, HS_ERR_INVALID, "lanes must be 1 or 2");
    HIP_TRY(h, hipSetDevice(h->device));
    if (lanes == 1) { if (h->lane2) { hs_orb_destroy(h->lane2); h->lane2 = nullptr; } return HS_OK; }
    if (!h->lane2) {
        int rc = hs_orb_create(&h->p, h->device, &h->lane2);
        if (rc != HS_OK) return hs_fail(h, rc, "could not create the second lane");
        if (!h->ev_fork) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        if (!h->ev_join) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    }
    return HS_OK;
}

int hs_orb_set_split(hs_orb* h, int mode)
{
    if (!h) return HS_ERR_INVALID;
    if (mode < -1 || mode > 1) return hs_fail(h, HS_ERR_INVALID, "split mode must be -1 (auto), 0 or 1");
    h->knobs.split_mode = mode;
    if (h->lane2) h->lane2->knobs.split_mode = mode;
    return HS_OK;
}

int hs_orb_synchronize(hs_orb* h, void* stream)
{
    if (!h) return HS_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(hs_stream_or(h, stream)));
    return HS_OK;
}

int hs_orb_debug_level(hs_orb* h, int image, int level, uint8_t* out, size_t cap_bytes, int32_t* lw, int32_t* lh)
{
    if (!h) return HS_ERR_INVALID;
    if (!out || image < 0 || image >= h->geo.last_batch || level < 0 || level >= h->p.nlevels) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    const HsLevel& V = h->geo.lv[level];
    if ((size_t)V.w * V.h > cap_bytes) return hs_fail(h, HS_ERR_CAPACITY, "level larger than buffer");
    if (lw) *lw = V.w;
    if (lh) *lh = V.h;
    const uint8_t* src; size_t pitch;
    if (level == 0) { src = hs_img0_ptr(h->geo.last_img0, image); pitch = h->geo.last_img0.row_stride; }
    else { src = V.base + (size_t)image * V.img_stride; pitch = V.pitch; }
    HIP_TRY(h, hipMemcpy2D(out, V.w, src, pitch, V.w, V.h, hipMemcpyDeviceToHost));
    return HS_OK;
}

int hs_orb_set_debug(hs_orb* h, int on)
{
    if (!h) return HS_ERR_INVALID;
    h->keep_points = on != 0;
    if (h->lane2) h->lane2->keep_points = h->keep_points;
    return HS_OK;
}

int hs_orb_debug_candidates(hs_orb* h, int image, int level, int32_t* xys, int cap, int32_t* n)
{
    if (!h) return HS_ERR_INVALID;
    if (h->knobs.fast_keys && h->geo.last_batch <= h->knobs.fast_keys_max_batch && !h->keep_points)
        return hs_fail(h, HS_ERR_INVALID, "hs_orb_debug_candidates: call hs_orb_set_debug(h, 1) before the extraction (the candidates are only gathered into a dense list in debug mode)");
    if (!xys || !n || image < 0 || image >= h->geo.last_batch || level < 0 || level >= h->p.nlevels) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    const HsLevel& V = h->geo.lv[level];
    int32_t cnt = 0;
    HIP_TRY(h, hipMemcpy(&cnt, h->geo.d_cand_count + image * h->p.nlevels + level, 4, hipMemcpyDeviceToHost));
    cnt = std::min(cnt, V.cand_cap);
    *n = cnt;
    if (cnt > cap) return hs_fail(h, HS_ERR_CAPACITY, "more candidates than buffer");
    std::vector<uint32_t> xy(cnt), sk(cnt);
    if (cnt) {
        HIP_TRY(h, hipMemcpy(xy.data(), h->geo.d_pts_xy + (size_t)image * h->geo.cand_img_stride + V.cand_off, (size_t)cnt * 4, hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(sk.data(), h->geo.d_pts_sk + (size_t)image * h->geo.cand_img_stride + V.cand_off, (size_t)cnt * 4, hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < cnt; i++) { xys[3 * i] = xy[i] & 0xFFFF; xys[3 * i + 1] = xy[i] >> 16; xys[3 * i + 2] = sk[i] >> 24; }
    return HS_OK;
}

int hs_orb_debug_selected(hs_orb* h, int image, int level, int32_t* xys, int cap, int32_t* n)
{
    if (!h) return HS_ERR_INVALID;
    if (!xys || !n || image < 0 || image >= h->geo.last_batch || level < 0 || level >= h->p.nlevels) return hs_fail(h, HS_ERR_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    const HsLevel& V = h->geo.lv[level];
    int32_t cnt = 0;
    HIP_TRY(h, hipMemcpy(&cnt, h->geo.d_sel_count + image * h->p.nlevels + level, 4, hipMemcpyDeviceToHost));
    *n = cnt;
    if (cnt > cap) return hs_fail(h, HS_ERR_CAPACITY, "more keypoints than buffer");
    if (cnt) HIP_TRY(h, hipMemcpy(xys, h->geo.d_sel + ((size_t)image * h->geo.sel_img_stride + V.sel_off) * 3, (size_t)cnt * 12, hipMemcpyDeviceToHost));
    return HS_OK;
}

int hs_orb_debug_quadtree_replay(hs_orb* h, int level_first, int level_count, int threads, int reps, float* ms_per_launch)
{
    if (!h) return HS_ERR_INVALID;
    const int L = h->p.nlevels, batch = h->geo.last_batch;
    if (!ms_per_launch || batch <= 0 || level_first < 0 || level_count < 1 || level_first + level_count > L || reps < 1 || (threads != 0 && threads != 256 && threads != 512))
        return hs_fail(h, HS_ERR_INVALID, "bad argument");
    if (threads != 0 && (h->qt_large || level_first < hs_quadtree_small_from(h->geo.lv.data(), L))) return hs_fail(h, HS_ERR_INVALID, "hs_orb_debug_quadtree_replay: a level of the range does not fit the level instance");
    // with the keys the quadtree launch consumes (and zeroes) what the FAST launch left: only a call that ran without them can be replayed
    if (h->knobs.fast_keys && h->geo.d_fast_qt.p != nullptr && batch <= h->knobs.fast_keys_max_batch)
        return hs_fail(h, HS_ERR_INVALID, "hs_orb_debug_quadtree_replay: the last call ran with the FAST keys (HS_FAST_KEYS=0, or more frames per call than HS_FAST_KEYS_MAX_BATCH)");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    hs_orb::Geometry& g = h->geo;
    const HsLevel* const d_lv = h->d_lv + (hs_fast_narrow(h->knobs, g.fast_items_n, batch) ? L : 0);
    hipEvent_t e0, e1;
    HIP_TRY(h, hipEventCreate(&e0));
    HIP_TRY(h, hipEventCreate(&e1));
    (void)hipEventRecord(e0, h->stream);
    for (int r = 0; r < reps; r++)
        hs_launch_quadtree(d_lv, L, batch, g.total_cells, g.d_cand, g.d_cell_count, g.cand_img_stride, g.d_pts_xy, g.d_pts_sk, g.d_pt_node, g.d_cand_count,
                           g.d_sel, g.d_sel_count, g.sel_img_stride, g.d_sel_perm, h->knobs.qt_point_domain ? 1 : 0, level_first, level_count,
                           nullptr, g.d_qbest, g.qhist_stride, g.qbest_stride, h->keep_points ? 1 : 0, threads == 256 ? 3 : (threads == 512 ? 4 : (h->qt_large ? 2 : (h->qt_small_ok ? 1 : 0))), g.d_qt_rects, h->stream);
    (void)hipEventRecord(e1, h->stream);
    const hipError_t e = hipEventSynchronize(e1);
    float t = 0.f;
    if (e == hipSuccess) (void)hipEventElapsedTime(&t, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    HIP_TRY(h, e);
    HIP_TRY(h, hipGetLastError());
    *ms_per_launch = t / (float)reps;
    return HS_OK;
}

} // extern "C"
