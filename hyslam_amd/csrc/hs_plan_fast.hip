// hs_plan_fast.hip — the FAST stage's host plan (hs_fast.h, hs_plan.h): how a level's cells are grouped into work items, both item lists of a
// geometry, and the launch plan — tile width, tile rows, LDS layout, workgroups, spill areas and the work-unit schedule of one launch.  Pure host
// code: no HIP call, no handle, no kernel; kernels_fast.hip reads the records made here and nothing else.
#include "hs_plan.h"
#include <cstring>
#include <utility>

// Cells per work item for a level: as many as fit the tile (<= FR_MAXG), spread evenly over the row.  A tile row holds 4*COLS bytes starting at the
// item's first column rounded DOWN to a dword (a0 = iniX & ~3: the staging loads are dword-aligned), so an item of n cells fits when
//     (iniX & 3) + n * wcell + 6 <= 4*COLS        for every item of the row (iniX = HS_BORDER + first cell * wcell)
// and its corners fit the score tile's 8-bit column (one spare column per cell: column = 1 + px + cell <= 255).  Round 5: the test is made with
// the items' REAL offsets instead of the worst one (3): the standard geometry (cells of 31 px) takes 8 cells per item instead of 7 — 8 * 31 is
// a multiple of 4, every item starts on a dword — which is 12 % fewer items per frame (861 instead of 975 at 1080p / 1.2), each scanning the
// same 256 columns: the lanes of a scan block that hold interior pixels go from 86 % to 97 %.
// Tile width: LC = 6 (64 dwords: the throughput shape) or LC = 5 (32 dwords, two half-waves on different rows).  A geometry keeps BOTH item lists;
// hs_fast_narrow picks per call (narrow items for small batches, where the launch lasts as long as its slowest wave and twice as many,
// half as long items are what shortens it).
int hs_fast_max_cell_w(int lc) { return 4 * (1 << lc) - 9; }      // a single cell at the worst offset
int hs_fast_group_cells(int wcell, int ncols, int lc)
{
    if (wcell <= 0 || ncols <= 0) return 0;
    const int tile_w = 4 * (1 << lc);
    auto fits = [&](int g) {
        if (g * wcell + g > 256) return false;                                   // score tile column 1 + px + cell of the last corner
        for (int j0 = 0; j0 < ncols; j0 += g) {
            const int n = std::min(g, ncols - j0);
            if (((HS_BORDER + j0 * wcell) & 3) + n * wcell + 6 > tile_w) return false;
        }
        return true;
    };
    const int gcap = std::max(1, std::min(FR_MAXG, (tile_w - 6) / wcell));
    for (int ngroups = (ncols + gcap - 1) / gcap; ngroups <= ncols; ngroups++) {
        const int g = (ncols + ngroups - 1) / ngroups;                              // even spread over `ngroups` items
        if (fits(g)) return g;
    }
    return 1;                                                                       // plan_levels rejects wcell > hs_fast_max_cell_w(6), and no narrow list is built for wcell > hs_fast_max_cell_w(5)
}

namespace {

// what k_fast_rows assumes of an item: its tile row (offset + interior + 6 px of apron) inside the 4 << lc bytes of an LDS row, at most FR_MAXG cells, the last
// corner's score-tile column (1 + px + cell) in 8 bits, at most 64 dwords per row.  Checked for every item of both lists.
bool item_fits(const HsFastItem& it, int lc)
{
    if (it.th == 0) return true;                                                 // yields nothing; staged from (0, 0)
    const int tile_w = 4 << lc;
    return it.off < 4 && (int)it.off + (int)it.iw + 6 <= tile_w && (int)it.ndw * 4 <= tile_w && it.ncell >= 1 && it.ncell <= FR_MAXG && (int)it.iw + (int)it.ncell <= 256;
}

void build_items(const HsLevel* h_lv, int nlevels, HsFastItem* out /*[sum ngroups*nrows]*/)
{
    for (int l = 0; l < nlevels; l++) {
        const HsLevel& L = h_lv[l];
        for (int ci = 0; ci < L.nrows; ci++)
            for (int gj = 0; gj < L.ngroups; gj++) {
                HsFastItem& it = out[L.item_begin + ci * L.ngroups + gj];
                memset(&it, 0, sizeof(it));
                const int j0 = gj * L.grp_cells, ncell = std::min(L.grp_cells, L.ncols - j0);
                const int xoff = j0 * L.wcell, yoff = ci * L.hcell;
                const int iniX = HS_BORDER + xoff, iniY = HS_BORDER + yoff;
                const int maxX = std::min(iniX + ncell * L.wcell + 6, L.w - HS_BORDER), maxY = std::min(iniY + L.hcell + 6, L.h - HS_BORDER);
                const int tw = maxX - iniX, th = maxY - iniY;
                const bool valid = tw >= 7 && th >= 7;            // reference skip rules (:435,444) / cv::FAST on < 7 rows or columns
                const int a0 = iniX & ~3;
                it.base = l == 0 ? nullptr : L.base; it.img_stride = L.img_stride; it.pitch = L.pitch;
                it.c0 = ci * L.ncols + j0; it.gcell0 = L.cell_begin + it.c0;
                it.ccap = hs_cell_cap(L.wcell, L.hcell);
                it.slot0 = (uint32_t)(L.cand_off + (uint64_t)it.c0 * it.ccap);
                it.inv_w = L.inv_wcell; it.inv_w1 = L.inv_wcell1;
                it.iniY = valid ? (uint16_t)iniY : 0; it.a0 = valid ? (uint16_t)a0 : 0;   // invalid items still prefetch (harmlessly) from (0,0)
                it.th = valid ? (uint16_t)th : 0; it.iw = valid ? (uint16_t)(tw - 6) : 0;
                it.off = (uint8_t)(iniX - a0); it.ndw = valid ? (uint8_t)((iniX - a0 + tw + 3) >> 2) : 1;
                it.ncell = (uint8_t)ncell; it.level = (uint8_t)l;
                it.xoff = (uint16_t)xoff; it.yoff = (uint16_t)yoff;
            }
    }
}

// Order of the FAST work items of an image: the REDUCED levels first, deepest level first, level 0 last.  An item of a reduced level
// costs 2-3 times an item of level 0 (the same number of pixels, denser corners), and the persistent FAST kernel walks the items in this
// order: with the cheap, uniform level-0 items at the end of every queue the tail of the launch — waves finishing their last item while
// the queues are empty — is short (a 32-frame launch spent ~17 % more per frame than a 128-frame launch with the expensive items last).
int order_items(std::vector<HsLevel>& lv, int fast_order)
{
    const int L = (int)lv.size();
    int pos = 0;
    if (fast_order == 0) { for (int l = 0; l < L; l++) { lv[l].item_begin = pos; pos += lv[l].ngroups * lv[l].nrows; } }
    else {
        for (int l = L - 1; l >= 1; l--) { lv[l].item_begin = pos; pos += lv[l].ngroups * lv[l].nrows; }
        lv[0].item_begin = pos; pos += lv[0].ngroups * lv[0].nrows;
    }
    return pos;
}

// a launch of tile width `lc` over `item_count` of the `items_all` items of every image
HsFastLaunch launch_plan(const HsKnobs& k, int max_hcell, int lc, int items_all, int batch, int item_first, int item_count, int spill_slot)
{
    HsFastLaunch P{};
    P.lc = lc; P.narrow = lc == 5;
    const int cols = 1 << lc, pitch = 4 * cols + FR_PAD;
    // Tile rows = the tallest tile of the launch
#define HS_TR_ENTRY(TR_) TR_,
    static const int TILE_ROWS[] = { HS_FAST_TILE_ROWS(HS_TR_ENTRY) };
#undef HS_TR_ENTRY
    for (const int tr : TILE_ROWS) { P.tr = tr; if (max_hcell + 6 <= tr) break; }
    FastRowsLds& L = P.lds;
    // LDS is granted in 1280-byte granules on gfx950 (160 KB / 128), and a persistent grid sized for more workgroups per CU than really fit runs its
    // surplus in a second round (measured: +25 % kernel time).  The kernel is latency-bound — measured at 6 / 8 / 11 workgroups per CU (wide items, 128
    // frames): 0.801 / 0.661 / 0.546 ms = 0.240 + 3.37 / n — so a workgroup more per CU is worth more than a long list as long as the list of the
    // TALLEST item keeps `min_entries` (a list of 624 instead of 1056 entries cost 4 % at equal occupancy, one of 800 1.6 %: shorter items, whose
    // list starts where their tile ends, keep 800-900).  Wide tiles of 40 rows: 10 granules = 12 800 bytes = 12 per CU (round 4: 14 080 = 11).
    constexpr int GRAN = 1280, LDS_CU = 160 * 1024;
    const int cnt_bytes = 4 * FR_MAXG;
    const int rs = 64 / cols, blk_rows = 8 * rs;
    const int over_rows = blk_rows * ((P.tr - 6 + blk_rows - 1) / blk_rows) + 6;      // the last scan block of a lane reads whole blocks: up to this many tile rows (the extra ones are masked out)
    // floor: one row step of a scan block (64 lanes x 4 pixels, whatever the tile width) must fit an empty list — the scored corners leave
    // their scores in `pscore` while the rest of the list is still being read, so the list may never run past its end
    const int min_entries = std::max(256, k.fast_list_min > 0 ? k.fast_list_min : 608);
    const int floor_bytes = std::max(P.tr * pitch + 3 * (min_entries + 16) + cnt_bytes, over_rows * pitch);
    int granules = (floor_bytes + GRAN - 1) / GRAN;
    while (LDS_CU / (granules * GRAN) > 16 && LDS_CU / ((granules + 1) * GRAN) >= 16) granules++;      // at most 16 workgroups per CU anyway (narrow tiles: 4 waves per SIMD by registers): the list takes the LDS that would stay unused
    L.total = granules * GRAN;
    L.off_cnt = L.total - cnt_bytes;
    L.pcap_min = ((L.off_cnt - P.tr * pitch) / 3) & ~15;       // list entries of the tallest item (2 bytes position + 1 byte score each)
    L.pcap_max = k.fast_small_lists ? 256 : k.fast_pcap > 0 ? std::max(256, k.fast_pcap & ~15) : (1 << 20);
    int per_cu = std::max(1, std::min(16, LDS_CU / ((L.total + GRAN - 1) / GRAN * GRAN)));
    if (k.fast_wg_per_cu > 0) per_cu = std::max(1, std::min(per_cu, k.fast_wg_per_cu));
    P.ovf_stride = (uint32_t)((4 * cols - 6) * std::max(max_hcell, 1));       // every interior pixel of an item a corner

    // workgroups of a launch over `work` units (non-decreasing in `work`)
    auto grid = [&](int work) {
        int nblk = (256 * per_cu) & ~(HS_FAST_NQ_MAX - 1);         // a multiple of every queue count
        while (nblk >= 2 * HS_FAST_NQ_MAX && (nblk / 2) % HS_FAST_NQ_MAX == 0 && nblk / 2 >= work) nblk /= 2;   // tiny jobs: fewer idle workgroups
        return nblk;
    };
    P.item_first = item_first; P.items_per_img = item_count; P.total_work = item_count * batch;
    P.nblk = grid(P.total_work);
    P.spill_base = (uint32_t)spill_slot * (uint32_t)grid(items_all * batch) * P.ovf_stride;      // the largest grid this geometry and batch may see
    P.force_scan_b = k.fast_scan_b;

    // queue count and unit order (see FastSched)
    FastSched& S = P.S;
    const int nq_want = k.fast_nq > 0 ? k.fast_nq : HS_FAST_NQ_MAX;
    int nq_log = 3;
    while ((2 << nq_log) <= nq_want) nq_log++;
    const int nq = 1 << nq_log;
    S.nq_log = nq_log;
    if (!k.fast_no_fold && !k.fast_image_major && batch > 0 && (long long)item_count * batch <= 2LL * P.nblk) { S.nq_log = 3; S.mode = 4; S.par = batch; S.per_q = item_count * batch; }
    else if (!k.fast_image_major && batch >= nq && batch % nq == 0) { S.mode = 1; S.par = batch / nq; S.per_q = S.par * item_count; }
    else if (!k.fast_image_major && batch > 0 && nq % batch == 0) {
        S.mode = 2; S.par = nq / batch;
        while ((1 << S.par_log) < S.par) S.par_log++;
        S.per_q = (item_count + S.par - 1) / S.par;
    } else if (!k.fast_image_major && batch > 0) { S.mode = 3; S.par = batch; S.per_q = (item_count * batch + nq - 1) / nq; }
    else { S.mode = 0; S.per_q = (item_count * batch + nq - 1) / nq; }
    auto magic = [](int d) { return d > 1 ? (uint32_t)(((1ull << 32) + (uint64_t)d - 1) / (uint64_t)d) : 0u; };       // ceil(2^32 / d); d <= 1: unused (fast_div)
    S.m_per_q = magic(S.per_q); S.m_par = magic(S.par); S.m_items = magic(item_count);
    return P;
}

} // namespace

// Both FAST work-item lists, in the order of order_items.  The narrow list: the same levels with NARROW work items (tiles of 32 dwords: <= 119 px of
// interior per item), for the launches of small batches: it differs in the grouping of the cells only, so everything downstream of the FAST kernel
// (the quadtree's gather) reads the grouping it was launched with from ITS copy of the level array (lv_n).  The plan's last step: build_items copies
// HsLevel::base (here: the level's offset), and the narrow levels are a copy of the finished wide ones.
const char* hs_plan_fast_items(const HsKnobs& k, HsPlan& P)
{
    const int L = (int)P.lv.size();
    order_items(P.lv, k.fast_order);
    P.lv_n = P.lv;
    bool narrow_ok = k.fast_cols != 64;
    for (int l = 0; l < L; l++) if (P.lv[l].wcell > hs_fast_max_cell_w(5)) narrow_ok = false;
    if (narrow_ok) {
        for (int l = 0; l < L; l++) {
            HsLevel& V = P.lv_n[l];
            V.grp_cells = hs_fast_group_cells(V.wcell, V.ncols, 5);
            V.ngroups = V.grp_cells > 0 ? (V.ncols + V.grp_cells - 1) / V.grp_cells : 0;
        }
        P.fast_items_n = order_items(P.lv_n, k.fast_order);
    }
    bool items_fit = true;                                 // every item against the tile the kernel stages it into (item_fits: columns, score-tile column, cells)
    auto build = [&](const std::vector<HsLevel>& lv, int n_items, std::vector<HsFastItem>& fi, int lc) {
        fi.assign(std::max(n_items, 1), HsFastItem{});
        build_items(lv.data(), L, fi.data());
        for (int i = 0; i < n_items; i++) items_fit = items_fit && item_fits(fi[i], lc);
        if (k.fast_order == 2 && L > 2) {                  // experiment: the reduced levels interleaved in proportion (every stretch of the list has the same mix of levels), level 0 last
            const int n_red = lv[0].item_begin;
            std::vector<std::pair<double, int>> key(n_red);
            for (int l = 1; l < L; l++) {
                const int n = lv[l].ngroups * lv[l].nrows;
                for (int j = 0; j < n; j++) key[lv[l].item_begin + j] = { (j + 0.5) / n, lv[l].item_begin + j };
            }
            std::stable_sort(key.begin(), key.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first < b.first; });
            std::vector<HsFastItem> t(fi.begin(), fi.begin() + n_red);
            for (int i = 0; i < n_red; i++) fi[i] = t[key[i].second];
        }
    };
    build(P.lv, P.fast_items, P.items, 6);
    if (P.fast_items_n > 0) build(P.lv_n, P.fast_items_n, P.items_n, 5);
    return items_fit ? nullptr : "internal: a FAST work item does not fit its tile (hs_fast_group_cells); geometry refused";
}

bool hs_fast_narrow(const HsKnobs& k, int items_narrow, int batch)
{
    const int narrow_max = k.fast_narrow_max > 0 ? k.fast_narrow_max : 18000;
    return items_narrow > 0 && (k.fast_cols == 32 || (k.fast_cols != 64 && (long long)items_narrow * batch <= narrow_max));
}

HsFastLaunch hs_fast_launch_plan(const HsKnobs& k, int max_hcell, int items_wide, int items_narrow, int batch, int item_first, int item_count, int spill_slot)
{
    const bool narrow = hs_fast_narrow(k, items_narrow, batch);
    return launch_plan(k, max_hcell, narrow ? 5 : 6, narrow ? items_narrow : items_wide, batch, item_first, item_count, spill_slot);
}

size_t hs_fast_overflow_bytes(const HsKnobs& k, int max_hcell, int items_wide, int items_narrow, int batch)
{
    const int n = std::max(items_wide, items_narrow);
    size_t spill = 0;                                             // either tile width may be launched on this workspace, and two launches may be in flight:
    for (int lc = 5; lc <= 6; lc++)                               // two full-size halves, the second of which starts at spill slot 1's base
        spill = std::max(spill, (size_t)2 * launch_plan(k, max_hcell, lc, n, batch, 0, n, 1).spill_base * 4);
    return (size_t)4 * HS_FAST_QUEUE_DWORDS * 4 + spill;
}
