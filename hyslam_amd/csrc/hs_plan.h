// hs_plan.h — the extractor's configuration as a pure host computation (hs_plan.hip, the pyramid's part in hs_plan_pyramid.hip, the FAST stage's in hs_plan_fast.hip): everything hs_orb_reserve decides for one frame size,
// without a HIP call and without the handle.  hs_api.hip allocates from the plan's sizes, uploads its arrays and turns its offsets into pointers.
#pragma once
#include "hs_internal.h"

// The handle's tuning / parity-test knobs of the environment, read ONCE per handle by hs_read_knobs (hs_api.hip: the table of names, defaults and
// meanings is there; INTEGRATION.md lists them for users).  Flags are 0 / 1.  HS_PYRAMID_NW8 (kernels_pyramid.hip) is read where it is used.
struct HsKnobs {
    int no_fuse, stereo_fuse, stereo_kpw, fast_keys, fast_keys_levels, fast_keys_max_batch, fast_order;
    int fast_pcap, fast_list_min, fast_small_lists, fast_wg_per_cu, fast_scan_b, fast_image_major, fast_nq, fast_cols, fast_narrow_max, fast_no_fold;   // the FAST launch plan's (hs_plan_fast.hip)
    int chain_mode, pyr_chain2, pyr_tbx_max, deep_max_batch, deep_rows;
    int qt_point_domain, qt_small, qt_small_from, qt_small_threads, split_mode;
    bool pyr_plan_set = false;         // HS_PYRAMID_PLAN is in the environment (an empty string is a plan too: no chain at all)
    std::string pyr_plan;
};
HsKnobs hs_read_knobs();              // hs_api.hip: every row of the table from the environment

// What the plan is made from: the extractor's parameters, its constructor tables (ORBExtractor.cpp:86-118), the knobs and the frame size.
struct HsPlanInput {
    const hs_orb_params* p;
    const float* inv_scale; const float* scale; const int* quota;      // [nlevels]
    const HsKnobs* knobs;
    bool qt_large;
    int w, h;
};

// The plan of one frame size, independent of the batch and free of addresses.  Every pointer field of its records holds a BYTE OFFSET into the
// buffer the field will point into, until hs_api.hip relocates it:
//   HsLevel::base, HsFastItem::base, HsPyrFuse::{s,a,b}base, HsPyrChain::sbase, HsPyrStage::base   -> one image's pyramid (d_pyr)
//   HsLevel::{xofs,ialpha,yofs,ibeta}, HsPyrFuse::xtA/xtB, HsPyrStage::xt                          -> tables (d_tables)
//   HsLevel::qt_xtab/qt_ytab -> qt_tabs;   HsFastQt::xkey/ykey -> qkeys;
//   HsPyrFuse::row*/xt/yt, HsPyrStage::rows/tx/ty -> pyr_tabs;   HsPyrFuseCols, HsPyrChainCols, pyr_level_cols -> pyr_cols
// Offset 0 is a valid place (level 1 starts one image's pyramid), so "none" is never told from the field's value: level 0 has no pyramid buffer
// and no resize tables, a fused pair / chain that starts at level 1 reads the caller's frames (sbase stays nullptr), a level has quadtree
// tables iff qt_ytab != 0 (the y table follows the x table), a HsFastQt record iff enabled, a pyramid record iff valid.
struct HsPlan {
    int w = 0, h = 0;
    int total_cells = 0, max_wcell = 1, max_hcell = 1, fast_items = 0, fast_items_n = 0;
    uint64_t cand_img_stride = 0; int sel_img_stride = 0, max_kp = 0;
    uint32_t qhist_stride = 0, qbest_stride = 0;
    size_t pyr_per_img = 0;                    // bytes of one image's levels 1.., a multiple of 256
    std::vector<HsLevel> lv, lv_n;             // the levels with the wide / the narrow FAST work items
    std::vector<int16_t> tables;               // cv::resize tables of every level >= 1
    std::vector<uint8_t> qt_tabs;              // geometric-key tables of the count-domain quadtree
    std::vector<uint16_t> qkeys;               // the FAST kernel's u16 key tables
    std::vector<HsFastQt> fast_qt;             // [nlevels]
    std::vector<uint64_t> pyr_tabs;            // tile / row records of the fused and chain pyramid kernels
    std::vector<uint64_t> pyr_cols;            // column records (HsPyrCol) of the LDS-staged pyramid kernels: HS_PYR_COL_TILE_BYTES (3 KiB) per tile column, one set per fused pair
                                               // and level, per chain stage and per level on its own (1080p, 8 levels: 132 tile columns, 396 KiB).  Derived from `tables` and
                                               // the tile records, hence not part of the digest (hs_plan_digest)
    std::vector<HsPyrFuseCols> pyr_fuse_cols;  // [level]: where the records of pyr_fuse[level] are
    std::vector<HsPyrChainCols> pyr_chain_cols, pyr_deep_cols;   // [level]: the same for pyr_chain / pyr_deep, per stage
    std::vector<HsPyrFuse> pyr_fuse;           // [level]: the pair (level, level + 1) when it is fused
    std::vector<HsPyrChain> pyr_chain;         // [level]: the chain launch that starts at this level (HsLevel::chain_n levels)
    std::vector<HsPyrChain> pyr_deep;          // [level]: the small-batch plan; valid = 0 where no chain starts
    std::vector<const uint8_t*> pyr_level_cols;// [level]: column records of the level made on its own (k_resize_level_lds); level 0 has none
    std::vector<HsFastItem> items, items_n;    // one image's FAST work items, wide / narrow (items_n: fast_items_n > 0); at least one record each
    uint64_t digest = 0;                       // hs_plan_digest of all of the above but the column records
};

// HS_OK and the plan, or the status and the text of a refusal (the plan is then unspecified)
int hs_plan_geometry(const HsPlanInput& in, HsPlan& out, std::string& err);
// its pyramid step (hs_plan_pyramid.hip), after the levels and the resize tables: the fused pairs, the chains, the small-batch plan and their records
void hs_plan_pyramid(const HsKnobs& k, HsPlan& P);
// its last step (hs_plan_fast.hip): the order of an image's FAST work items and both item lists; nullptr, or the text of the refusal (HS_ERR_INVALID)
const char* hs_plan_fast_items(const HsKnobs& k, HsPlan& P);
// FNV-1a-style 64-bit hash (xor, multiply by the FNV prime; 8-byte words where possible) over the plan, field by field in the order stated at its definition: equal digests <=> the kernels get the same tables,
// records and launch geometry
uint64_t hs_plan_digest(const HsPlan& P);

// The quadtree kernel's LEVEL instance (kernels_quadtree.hip: eight waves — or four — and 39 KB of LDS per workgroup, four workgroups per CU) sizes its scratch
// by these instead of by the largest level any configuration may have.  Launch modes 3 / 4 of hs_launch_quadtree (256 / 512 threads) select it; a
// launch that passes the FAST kernel's key histogram ignores them (the histogram is one level deeper than the instance's pyramid).
#define HS_QT_LEVEL_NODES 512      // list capacity (>= quota + 8)
#define HS_QT_LEVEL_XTAB 2048      // bytes of the x key table in LDS (>= qt_w + 1)
#define HS_QT_LEVEL_YTAB 1024      // ... of the y key table (>= qt_h + 1)
#define HS_QT_LEVEL_TILES 256      // 64-px tiles of the spatial order
#define HS_QT_LEVEL_HPYR 2736      // histogram pyramid entries: n_ini * (4^(DH+1) - 1) / 3 <= 2730 for (n_ini <= 2, DH = 5) and (n_ini <= 8, DH = 4)
// true exactly when the level instance can take the level: quota + 8 list entries, both key tables, the tile counters and a histogram pyramid of
// depth >= 4 fit it.  A function of the level record alone: nothing of it enters the plan's digest.
bool hs_quadtree_small_level(const HsLevel& V);
// the first level from which EVERY level passes hs_quadtree_small_level (nlevels: none)
int hs_quadtree_small_from(const HsLevel* lv, int nlevels);
