// hs_work.h — the layout of every caller-owned work area (`d_work`) of the resident chain: one struct per area.  The struct's constructor walks a
// cursor over the caller's block once and fills the typed pointers; bytes() is the same walk without a block, so a size and its carve cannot
// disagree, and the hs_*_work_bytes of include/hyslam_amd.h are these bytes().  A nested area is the inner struct constructed from the outer
// cursor.  Host only and free of HIP: <cstddef> and <cstdint> are all it needs (tests/cpp/test_work_layout.cpp includes it alone).
// include/hyslam_amd.h promises a 16-byte aligned d_work and nothing more: offsets are rounded to 256, addresses are not.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef HS_LOCAL_POINTS_BLOCK          // include/hyslam_amd.h states it (a different value there is a redefinition: the compiler says so)
#define HS_LOCAL_POINTS_BLOCK 1024
#endif

inline size_t hs_up256(size_t v) { return (v + 255) & ~(size_t)255; }    // the library's one rounding helper
inline size_t hs_dim(int v) { return v > 0 ? (size_t)v : 0; }            // a negative dimension is an empty one

// A bump cursor over `base`.  Without a base it only counts: every address is formed from integers, so no arithmetic happens on a null pointer.
class HsWorkCursor {
public:
    HsWorkCursor() {}
    explicit HsWorkCursor(void* base) : base_(reinterpret_cast<uintptr_t>(base)) {}
    template <class T> T* take(size_t count) { T* p = reinterpret_cast<T*>(here()); off_ += count * sizeof(T); return p; }
    HsWorkCursor& align256() { off_ = hs_up256(off_); return *this; }
    void skip(size_t bytes) { off_ += bytes; }
    size_t offset() const { return off_; }
    void* here() const { return base_ ? reinterpret_cast<void*>(base_ + off_) : nullptr; }
private:
    uintptr_t base_ = 0; size_t off_ = 0;
};

// Every struct: `base` is the area's first byte, which is what the area's own entry point takes as d_work.  Each area ends in 256 spare bytes.

// replay in landmark order (hs_launch_frame_associate)
struct HsAssocWork {
    void* base; int32_t *minw, *maxw, *erased /*[n]*/, *jk /*[L]*/;
    HsAssocWork(HsWorkCursor& c, int n, int L)
        : base(c.here()), minw(c.take<int32_t>(hs_dim(n))), maxw(c.take<int32_t>(hs_dim(n))), erased(c.take<int32_t>(hs_dim(n))), jk(c.take<int32_t>(hs_dim(L)))
    { c.skip(256); }
    static size_t bytes(int n, int L) { HsWorkCursor c; HsAssocWork(c, n, L); return c.offset(); }
};

// replay in view order (hs_launch_frame_associate_views)
struct HsVassocWork {
    void* base; int32_t *view_op /*[n]*/, *lm_view, *idx_old /*[L]*/;
    HsVassocWork(HsWorkCursor& c, int n, int L)
        : base(c.here()), view_op(c.take<int32_t>(hs_dim(n))), lm_view(c.take<int32_t>(hs_dim(L))), idx_old(c.take<int32_t>(hs_dim(L)))
    { c.skip(256); c.align256(); }
    static size_t bytes(int n, int L) { HsWorkCursor c; HsVassocWork(c, n, L); return c.offset(); }
};

// local points (hs_launch_local_points): a flag byte per landmark, a count per block of HS_LOCAL_POINTS_BLOCK landmarks
struct HsLocalPointsWork {
    void* base; uint8_t* flag /*[L]*/; int32_t* block_cnt /*[n_blocks]*/; int n_blocks;
    static int blocks(int L) { return (int)((hs_dim(L) + HS_LOCAL_POINTS_BLOCK - 1) / HS_LOCAL_POINTS_BLOCK); }
    HsLocalPointsWork(HsWorkCursor& c, int L) : base(c.here()), n_blocks(blocks(L))
    {
        flag = c.take<uint8_t>(hs_dim(L)); c.align256();
        block_cnt = c.take<int32_t>((size_t)n_blocks); c.align256();
        c.skip(256);
    }
    static size_t bytes(int L) { HsWorkCursor c; HsLocalPointsWork(c, L); return c.offset(); }
};

// local map (hs_local_map_search_device): the vote's one query and its count of ordered slots in a 256-byte head, then local points
struct HsLocalMapWork {
    void* base; int64_t* q_off /*[2]*/; int32_t* n_ordered; HsLocalPointsWork points;
    HsLocalMapWork(HsWorkCursor& c, int L) : base(c.here()), q_off(c.take<int64_t>(2)), n_ordered(c.take<int32_t>(1)), points(c.align256(), L) {}
    static size_t bytes(int L) { HsWorkCursor c; HsLocalMapWork(c, L); return c.offset(); }
};

// track (hs_track_motion_model_device, hs_track_local_map_device): the replay, then the local map; a chain uses them one after the other
struct HsTrackWork {
    void* base; HsAssocWork assoc; HsLocalMapWork local_map;
    HsTrackWork(HsWorkCursor& c, int n, int L) : base(c.here()), assoc(c, n, L), local_map(c.align256(), L) { c.align256(); c.skip(256); }
    static size_t bytes(int n, int L) { HsWorkCursor c; HsTrackWork(c, n, L); return c.offset(); }
};

// initial pose estimation (hs_track_reference_keyframe_device, hs_track_initial_device, hs_track_normal_device): the tracking area first, so that the
// motion and local-map stages carve theirs from the same base; then the replay in view order and the search's ops as the gate masked them
struct HsInitialWork {
    void* base; HsTrackWork track; HsVassocWork vassoc; int32_t *op_view_run, *op_lm_run /*[n]*/;
    HsInitialWork(HsWorkCursor& c, int n, int L) : base(c.here()), track(c, n, L), vassoc(c.align256(), n, L)
    {
        op_view_run = c.take<int32_t>(hs_dim(n)); op_lm_run = c.take<int32_t>(hs_dim(n)); c.align256();
        c.skip(256);
    }
    static size_t bytes(int n, int L) { HsWorkCursor c; HsInitialWork(c, n, L); return c.offset(); }
};

// key frame (hs_keyframe_reference_device, hs_keyframe_create_device): the vote's query and its three scalars in a 256-byte head, the depth keys,
// the vote's counter row.  The caller sizes the row with kf_cap; hs_keyframe_reference_device votes over T->n_kf counters and has no way to check
// kf_cap >= T->n_kf: that is the caller's contract (include/hyslam_amd.h), and the entry points carve with T->n_kf, which moves no pointer.
struct HsKeyframeWork {
    void* base; int64_t* q_off /*[2]*/; int32_t* vote /*[3]*/; unsigned long long* keys /*[n]*/; int32_t* weights /*[kf_cap]*/;
    HsKeyframeWork(HsWorkCursor& c, int n, int kf_cap) : base(c.here()), q_off(c.take<int64_t>(2)), vote(c.take<int32_t>(3))
    {
        c.align256();
        keys = c.take<unsigned long long>(hs_dim(n)); c.align256();
        weights = c.take<int32_t>(hs_dim(kf_cap)); c.align256();
        c.skip(256);
    }
    static size_t bytes(int n, int kf_cap) { HsWorkCursor c; HsKeyframeWork(c, n, kf_cap); return c.offset(); }
};
