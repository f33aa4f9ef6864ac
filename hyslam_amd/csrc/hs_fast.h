// hs_fast.h — the FAST stage's records, limits and host interface: what the planner (hs_plan_fast.hip) makes, what the kernel and its launch
// function (kernels_fast.hip) read, and the one piece of code both sides run — the work-unit schedule.  Included by hs_internal.h after HsLevel and
// HsImg0, never on its own.
#pragma once

// One work item of the FAST kernel (kernels_fast.hip): `ncell` horizontally adjacent cells of one cell row.  Everything that does not
// depend on the image index is precomputed on the host, so a wave fetches an item's geometry with a single 64-byte scalar load.
struct HsFastItem {
    const uint8_t* base;           // level buffer; nullptr = level 0 (the caller's frame, HsImg0)
    uint64_t img_stride;           // bytes between images of the level buffer
    int32_t pitch;                 // row pitch of the level buffer (level 0: HsImg0::row_stride)
    int32_t gcell0;                // HsLevel::cell_begin + c0: first entry of the item in cell_count
    int32_t c0;                    // cell index (row-major within the level) of the item's first cell
    uint32_t slot0;                // HsLevel::cand_off + c0 * ccap: the first cell's slots in the candidate arrays
    int32_t ccap;                  // slots per cell
    int32_t inv_w, inv_w1;         // ceil(65536 / wcell), ceil(65536 / (wcell + 1))
    uint16_t iniY, a0;             // first tile row; first tile column rounded down to a dword
    uint16_t th, iw;               // tile rows (0: the item yields nothing), interior width
    uint8_t off, ndw, ncell, level;// tile column of x is off + (x - iniX); dwords per tile row
    uint16_t xoff, yoff;           // j0 * wCell, i * hCell (ORBExtractor.cpp:463-464)
    uint32_t _pad;
};
static_assert(sizeof(HsFastItem) == 64, "HsFastItem is fetched as one 64-byte record");

// Per-level record of the FAST kernel's key computation (one 32-byte scalar load per work item): u16 tables with the x part of a candidate's
// geometric key per pixel column — root << 2 DH | the column's cell index at depth DH with its bits spread to the even positions — and the y part
// per pixel row (bits spread to the odd positions), so that key = xkey[x] | ykey[y] (k_quadtree's geo_key, kernels_quadtree.hip); both padded
// by 512 entries so that a work item's slice can be fetched without clamping.
struct HsFastQt { const uint16_t* xkey; const uint16_t* ykey; uint32_t hist_off, best_off; int32_t enabled, _r; };
static_assert(sizeof(HsFastQt) == 32, "scalar-load record");

// candidate slots per FAST cell: 3x3 NMS leaves at most one survivor per 2x2 block; rounded to 4 so that a cell's records start on
// a 16-byte boundary (cand_off is a multiple of 4 entries)
__host__ __device__ inline int hs_cell_cap(int wcell, int hcell) { return ((((wcell + 1) >> 1) * ((hcell + 1) >> 1)) + 3) & ~3; }

#define HS_FAST_NQ_MAX 32          // work queues of the FAST kernel: 8, 16 or 32 (FastSched)
#define HS_FAST_QUEUE_DWORDS (32 * HS_FAST_NQ_MAX)   // head of the FAST overflow buffer: FOUR rotating sets of up to 32 work-queue counters on 128-byte lines of their own
#define FR_MAXG 8                  // cells per item (one per-cell counter each)
#ifndef FR_PAD
#define FR_PAD 16                  // row padding of the LDS tiles, bytes (multiple of 16)
#endif
// Tile rows held in LDS (6 + 8*RS*blocks): the instances of k_fast_rows, ascending.  A launch runs the smallest one that holds its tallest tile
// (max_hcell + 6 rows; HS_MAX_CELL_H + 6 <= the last): the planner's rounding and the launch function's dispatch both expand this list.
#define HS_FAST_TILE_ROWS(X) X(38) X(40) X(44) X(54) X(70) X(102) X(134)

// LDS of a workgroup: [0, th * PITCH) the item's pixel tile (later its score tile) | the pixel list of THIS item — 2 bytes of position + 1 byte of score per
// entry, as many entries as fit before the counters: an item of fewer rows than the tallest one of the launch has the longer list (round 5) | [off_cnt, total)
// the per-cell counters.  pcap_max: tuning / test cap on the list length (HS_FAST_PCAP, HS_FAST_TEST_SMALL_LISTS).  total = the launch's dynamic LDS bytes.
struct FastRowsLds { int32_t off_cnt, pcap_max, pcap_min, total; };

// How the work units of a launch are spread over the work queues (made by hs_fast_launch_plan).  The item list of an image is ordered expensive items
// first (the reduced levels, deepest first; level 0 last: hs_plan_fast.hip); a queue hands out its units in order, so its LAST units should be cheap —
// every wave still holds its current and its pre-grabbed next item when the queue runs dry, and with heavy items among them the launch ended with
// a third of its time spent draining (63 of 192 us at 32 frames; `tools/fast_wave_timeline.py`).  And there should be MANY queues: a queue is
// one counter, a counter serves same-address atomics one after the other, and with 8 of them for 30 000 items the grabs themselves were late
// (8 -> 32 queues: 0.175 -> 0.158 ms per 32 frames).
//   mode 1  the batch is a multiple of the queue count: a queue owns `par` whole images and walks them ITEM-major (item 0 of its images, item 1,
//           ...): its expensive items all go out early, its last units are the level-0 items of all its images
//   mode 2  the queue count is a multiple of the batch: an image is dealt round-robin to `par` queues (item i -> queue i % par), every one of
//           which sees the same mix of levels in the same order
//   mode 3  anything else: the item-major list of ALL images (item 0 of every image, item 1, ...) dealt round-robin to the queues
//   mode 0  contiguous ranges of the image-major order (HS_FAST_IMAGE_MAJOR=1: the scheme until the end of round 3, kept as a parity variant)
//   mode 4  FOLDED STATIC schedule for small launches (at most two units per workgroup; round 4): workgroup b takes unit b of the item-major
//           list of all images and then unit 2 * grid - 1 - b — the list is ordered expensive first, so the workgroups whose first item is the
//           cheapest get the (cheap) second items and the heaviest items run alone; no counter, no look-ahead grab.  At one stereo pair per
//           call the launch lasts as long as its slowest wave: with the look-ahead of the work queues the waves that started on the HEAVIEST
//           items were the first to grab a second one (`tools/fast_b1_timeline.py`: 28.8 us span, the slowest waves all "level 7 + another")
// The host half (mode, queue count, divisors) and the device half (the three functions below) meet only here; tests/test_fast_schedule.py runs both
// halves on the CPU and holds them to "every (item, image) exactly once".
struct FastSched { int32_t nq_log, mode, par, par_log, per_q; uint32_t m_per_q, m_par, m_items; };     // m_x = ceil(2^32 / x): fast_div()
// floor(a / d) for 0 <= a < 2^31 and d >= 1 with m = ceil(2^32 / d): the high product is floor(a / d) or one more (its error a * (m * d - 2^32) / (d * 2^32)
// is below a / 2^32 < 1/2), one compare corrects it.  Wave-uniform operands: two scalar multiplies instead of the ~20-instruction v_rcp_iflag sequence
// of an integer division, twice per work item on the critical path of every wave.
__host__ __device__ __forceinline__ int fast_div(int a, int d, uint32_t m)
{
#ifdef __HIP_DEVICE_COMPILE__
    int q = (int)__umulhi((uint32_t)a, m);
#else
    int q = (int)(((uint64_t)(uint32_t)a * m) >> 32);
#endif
    if (d == 1) q = a;                                          // (ceil(2^32 / 1) does not fit 32 bits)
    if (q * d > a) q--;
    return q;
}
// units of queue qq; queue qq hands out the units qq * per_q + [0, size)
__host__ __device__ __forceinline__ int fast_queue_size(const FastSched& S, int qq, int total_work, int items_per_img)
{
    if (S.mode == 1) return S.per_q;
    if (S.mode == 2) return (items_per_img - (qq & (S.par - 1)) + S.par - 1) >> S.par_log;
    if (S.mode == 3) return (total_work - qq + (1 << S.nq_log) - 1) >> S.nq_log;
    return min(max(total_work - qq * S.per_q, 0), S.per_q);
}
// work unit w -> (item of the launch's item list, image)
__host__ __device__ __forceinline__ int unit_decode(int items_per_img, const FastSched& S, int w, int* img)
{
    struct { int img; } g;
    int item;
    if (S.mode == 1) {
        const int q = fast_div(w, S.per_q, S.m_per_q), u = w - q * S.per_q;
        item = fast_div(u, S.par, S.m_par);
        g.img = q * S.par + (u - item * S.par);
    } else if (S.mode == 2) {
        const int q = fast_div(w, S.per_q, S.m_per_q), u = w - q * S.per_q;
        g.img = q >> S.par_log;
        item = (u << S.par_log) + (q & (S.par - 1));
    } else if (S.mode == 3) {
        const int q = fast_div(w, S.per_q, S.m_per_q), u = w - q * S.per_q, gidx = (u << S.nq_log) + q;      // position in the item-major list of all S.par images
        item = fast_div(gidx, S.par, S.m_par);
        g.img = gidx - item * S.par;
    } else if (S.mode == 4) {
        item = fast_div(w, S.par, S.m_par);                          // w = position in the item-major list of all S.par images
        g.img = w - item * S.par;
    } else {
        g.img = fast_div(w, items_per_img, S.m_items);
        item = w - g.img * items_per_img;
    }
    *img = g.img;
    return item;
}

// Everything one FAST launch decides, as a plain record: hs_fast_launch_plan (pure host code) makes it from the knobs, the geometry and the call;
// hs_launch_fast reads nothing else but buffers.
struct HsFastLaunch {
    int32_t lc, narrow;            // tile width: 6 / 5 = 64 / 32 dwords per tile row; narrow = 1: the launch reads the NARROW item list (HsPlan::items_n, lv_n)
    int32_t tr;                    // tile rows: the instance of HS_FAST_TILE_ROWS
    FastRowsLds lds;
    int32_t nblk;                  // workgroups: a multiple of every queue count
    uint32_t ovf_stride;           // dwords of a workgroup's spill area: every interior pixel of an item a corner
    uint32_t spill_base;           // spill slot 1: the second half starts after a full-size first one
    int32_t item_first, items_per_img, total_work;      // the launch covers items [first, first + items_per_img) of every image: total_work units
    int32_t force_scan_b;          // HS_FAST_TEST_SCAN_B
    FastSched S;
};

// hs_plan_fast.hip
struct HsKnobs;
int hs_fast_max_cell_w(int lc);                          // widest FAST cell the kernel's tile holds at any offset (247 px wide tiles, 119 px narrow ones); lc = 6 / 5: wide / narrow tiles
int hs_fast_group_cells(int wcell, int ncols, int lc);   // cells per FAST work item for a level (0 when the level has no cells)
// Item width by batch (round 4): a launch of few frames lasts as long as its slowest wave (one stereo pair: 1 904 wide items for 2 816 resident
// single-wave workgroups), so it gets the NARROW items — twice as many, half as long; measured at 1080p (pairs per call: narrow / wide pairs/s):
// 1: 9 949 / 8 403, 2: 16 029 / 15 642, 4: 23 004 / 22 660, 8: 32 657 / 33 240, 16: 40 917 / 41 507 — from ~18 k items on the wide ones win (fewer,
// fuller tiles).  HS_FAST_COLS = 32 / 64 forces one list, HS_FAST_NARROW_MAX moves the threshold.  items_narrow = 0: the geometry has no narrow list.
bool hs_fast_narrow(const HsKnobs& k, int items_narrow, int batch);
// the launch over items [item_first, item_first + item_count) of every image of the list hs_fast_narrow picks; spill_slot 0 / 1: which half of the
// spill areas (two launches of a handle may be in flight)
HsFastLaunch hs_fast_launch_plan(const HsKnobs& k, int max_hcell, int items_wide, int items_narrow, int batch, int item_first, int item_count, int spill_slot);
// work-queue counters + per-workgroup spill areas for any launch hs_fast_launch_plan can make on this geometry and batch
size_t hs_fast_overflow_bytes(const HsKnobs& k, int max_hcell, int items_wide, int items_narrow, int batch);

// kernels_fast.hip (asynchronous on `s`).  Returns whether a kernel was enqueued: a launch consumes one work-queue counter set (`epoch` & 3) and zeroes one
// for the launch after next, so the caller advances its epoch only for launches that happened
bool hs_launch_fast(const HsFastLaunch& P, const HsFastItem* d_items /*the list P.narrow names*/, HsImg0 img0, int fast_th,
                    uint2* cand /*{y<<16|x, score<<24|cell} per slot*/, int32_t* cell_count, uint64_t cand_img_stride, int total_cells,
                    uint32_t* overflow /*hs_fast_overflow_bytes(), its counter sets zero-initialised*/, uint32_t epoch /*launch counter of the handle*/,
                    const HsFastQt* d_qt /*[nlevels]; nullptr: no keys*/, uint32_t* qhist, unsigned long long* qbest, uint32_t qhist_img_stride, uint32_t qbest_img_stride, hipStream_t s);
