// hs_pyramid.h — the image pyramid's records, limits and host interface: what the planners (hs_plan_pyramid.hip) make, what the kernels and their
// launch function (kernels_pyramid.hip) read.  Included by hs_internal.h after HsLevel and HsImg0, never on its own.
#pragma once

// tile heights and the LDS pitch the planners and the kernels agree on
#define LT_ROWS 16                // destination rows per tile of k_resize_level_lds
#ifndef FZ_ROWS
#define FZ_ROWS 16                // level-B rows per tile of k_resize_two_levels; the default tile height of a chain's last level
#endif
#define FZ_APITCH 272             // LDS pitch of the level-A region: 256 columns + the 3-dword window over-read of the last lane

// Two-levels-per-launch pyramid kernel (kernels_pyramid.hip): everything a workgroup used to derive from the level and resize tables with a
// chain of dependent scalar loads is precomputed on the host — the tile geometry factorises into one record per tile column and one per tile
// row, the vertical pass gets one 8-byte record per destination row (clamped source rows + weights), and the level descriptions travel as a
// kernel argument instead of through the HsLevel array.
struct HsXTab { int16_t sx, a0, a1, pad; };                       // x table of cv::resize: first source column and the two 11-bit weights
struct HsPyrXTile { int32_t ax0, own_x1, col0, nvec, _r[4]; };    // first column / end of the owned columns of the level-A region; first source column (16-aligned), 16-byte vectors per source row
struct HsPyrYTile { int32_t ay0, own_y1, ay_last, sy_first, n_sr, _r[3]; };   // level-A rows [ay0, ay_last], owned up to own_y1; source rows from sy_first, n_sr of them
struct HsPyrRow { uint16_t off0, off1, b0, b1; };                 // a destination row OF ONE TILE: byte offsets of its two source rows in the tile's sums buffer ((row - first row held) * 512) and the vertical weights
static_assert(sizeof(HsPyrXTile) == 32 && sizeof(HsPyrYTile) == 32 && sizeof(HsPyrRow) == 8, "scalar-load records");
// Column record of one lane of a horizontal pass: what the LDS-staged kernels used to derive per workgroup from the four x-table entries of the lane
// (window position in the staged row, byte-pair selectors, coefficient pairs times 16).  It depends on the tile column and the lane only, so the plan
// makes it once (hs_pyramid_col_records).  In memory a tile column's 64 records are three planes of 64 x 16 bytes, so that every load of a wave is
// one contiguous KiB: plane 0 {wbase, wshift, sel[0], sel[1]}, plane 1 {sel[2], sel[3], coef[0], coef[1]}, plane 2 {coef[2], coef[3], 0, 0}.
struct HsPyrCol { int32_t wbase, wshift; uint32_t sel[4], coef[4]; };
#define HS_PYR_COL_TILE_BYTES 3072
struct HsPyrFuse {
    const uint8_t* sbase;          // source level S = A - 1 (nullptr: level 0 = the caller's frames, HsImg0)
    uint64_t s_img_stride; int32_t spitch; int32_t _r0;
    uint8_t* abase; uint64_t a_img_stride; int32_t apitch, aw, ah, slotA;   // slotA: records per y tile in rowA
    uint8_t* bbase; uint64_t b_img_stride; int32_t bpitch, bw, bh, _r2;
    const HsXTab* xtA; const HsXTab* xtB;
    const HsPyrRow* rowA; const HsPyrRow* rowB;                    // per y tile: [grid.y][slotA] rows ay0.. of the tile's level-A region, [grid.y][FZ_ROWS + 8] rows of its level-B tile (padded with copies of the last row)
    const HsPyrXTile* xt; const HsPyrYTile* yt;                    // [grid.x], [grid.y]
    int32_t tbx, sr, lds_pitch, valid;                             // tile width of level B, LDS rows / pitch of the source rectangle; valid = this pair is fused
};

// A CHAIN of 2 or 3 levels per launch (k_resize_chain: the two-level scheme applied once more, so that the last three levels of an 8-level
// pyramid are one launch instead of two).  Stage i produces level first+i from the LDS copy of the level before it (stage 0: from global
// memory); a workgroup owns one tile of the LAST level and, of every other level, the part induced by the tiles' first source columns / rows.
struct HsPyrStageX { int32_t x0, own_x1, ncols, src_x0, nvec, _r[3]; };      // region [x0, x0 + ncols) of the stage's level, owned up to own_x1; first column the source buffer holds; stage 0: 16-byte vectors per source row
struct HsPyrStageY { int32_t y0, own_y1, y_last, src_y0, n_src, _r[3]; };    // region rows [y0, y_last], owned up to own_y1; first row / number of rows the source buffer holds
static_assert(sizeof(HsPyrStageX) == 32 && sizeof(HsPyrStageY) == 32, "scalar-load records");
struct HsPyrStage {
    uint8_t* base; uint64_t img_stride; int32_t pitch, w, h, slot;           // the level the stage produces; slot = row records per y tile
    const HsXTab* xt; const HsPyrRow* rows;                                    // its x table and row records [grid.y][slot]: rows y0.. of the tile's region (padded with copies of the last row)
    const HsPyrStageX* tx; const HsPyrStageY* ty;                              // [grid.x], [grid.y]
};
#define HS_PYR_DEEP_LDS (120 * 1024)  // LDS a deep chain may plan with (hs_pyramid_plan_chain's lds_max for the small-batch plan)
#define HS_PYR_CHAIN_MAX 7            // levels one k_resize_chain launch can produce (small batches: the whole pyramid of 8 levels in ONE launch)
struct HsPyrChain {
    const uint8_t* sbase; uint64_t s_img_stride; int32_t spitch, nstage;       // the source level (sbase == nullptr: the caller's frames)
    HsPyrStage st[HS_PYR_CHAIN_MAX];
    int32_t tbx, lds_pitch, x_bytes, h_rows;                                   // tile width of the last level; LDS: pitch of the source rectangle, bytes of the level buffer, rows of the sums buffer
    int32_t grid_x, grid_y, valid, _r;
};

// Where the column records (HsPyrCol) of a launch are: kernel arguments beside HsPyrFuse / HsPyrChain, [grid.x] tile columns of HS_PYR_COL_TILE_BYTES each.
// They are derived data — a function of the x tables and the tile records — and live in a blob of their own (HsPlan::pyr_cols), so the records above and
// the plan's digest are what they were.
struct HsPyrFuseCols { const uint8_t* a; const uint8_t* b; };                  // level A (origin HsPyrXTile::col0), level B (origin HsPyrXTile::ax0)
struct HsPyrChainCols { const uint8_t* st[HS_PYR_CHAIN_MAX]; };                // per stage (origin HsPyrStageX::src_x0)
struct HsPyrCols { const HsPyrFuseCols* fuse; const HsPyrChainCols* chain; const HsPyrChainCols* deep; const uint8_t* const* level; };   // host arrays [nlevels]: beside fuse / chain / deep; a level made on its own (k_resize_level_lds)

// Dynamic LDS of a launch, for the planner's fit check and for the launch itself.  A fused pair: the source rectangle (sr rows of `pitch` bytes; the
// level-A region overlays it) and the 16-bit sums of max(sr, ar) rows of 256 columns.  A chain: the level buffer, rounded to 16 bytes (HsPyrChain::x_bytes
// is stored rounded), and the sums of h_rows rows.
inline size_t hs_pyr_fuse_lds(int pitch, int sr, int ar) { return (size_t)pitch * sr + (size_t)std::max(sr, ar) * 256 * 2; }
inline size_t hs_pyr_chain_lds(size_t x_bytes, int h_rows) { return ((x_bytes + 15) & ~(size_t)15) + (size_t)h_rows * 256 * 2; }

// kernels_pyramid.hip (asynchronous on `s`)
int  hs_launch_pyramid(const HsLevel* d_lv, const HsLevel* h_lv, const HsPyrFuse* fuse /*[nlevels], host*/, const HsPyrChain* chain /*[nlevels], host*/, int nlevels, HsImg0 img0, int batch, hipStream_t s,
                       const HsPyrCols& cols /*the launches' column records*/,
                       const HsPyrChain* deep = nullptr /*[nlevels], host: the small-batch plan (long chains); used where deep[l].valid*/);      // returns the kernel launches it enqueued
struct hs_orb;
struct HsDebugPyramidPlan { int nlevels; const HsLevel* lv; const HsPyrFuse* fuse; const HsPyrChain* chain; const HsPyrChain* deep; HsPyrCols cols; };   // [nlevels] each (host arrays, device addresses inside)
void hs_debug_pyramid_plan(const hs_orb* h, HsDebugPyramidPlan* out);      // hs_api.hip; everything null when nothing is configured
// hs_plan_pyramid.hip
// the 64 column records of one tile column (HsPyrCol, in the plane layout): lane t makes columns x0 + 4 t .. + 3 of a level of width w (columns past
// the last one repeat it), `origin` = first source column the staged rows hold; 384 words appended to `blob`, returns their byte offset
size_t hs_pyramid_col_records(const int16_t* xt /*{sx,a0,a1,-} per column*/, int w, int x0, int origin, std::vector<uint64_t>& blob);
// column records of a level made on its own: tile columns of 256, origin = the tile's first source column rounded down to 16 (k_resize_level_lds)
size_t hs_pyramid_level_cols(const int16_t* xt, int w, std::vector<uint64_t>& blob);
int hs_pyramid_launch_count(const HsLevel* h_lv, int nlevels);          // kernel launches of one hs_launch_pyramid call
