// kernels_fast.hip — K2+K3: FAST-9/16 corner detection, corner score and 3x3 non-max suppression, per cell.
//
// Replaces the per-cell loop of ORBExtractor::ComputeKeyPointsOctTree (src/features/ORBExtractor.cpp:430-470),
// which calls ORBFinder::detect = cv::FAST(cell, kps, 20, true) (src/features/low_level/ORBFinder.cpp:66-68)
// once per ~31x31 cell (6342 calls per 1080p frame).  Semantics that must hold for bit-exact keypoints:
//   * a cell's sub-image is its interior plus a 3 px apron; cell interiors tile [19,w-19) x [19,h-19);
//   * NMS is 3x3, strict, and *per cell*: a neighbour outside the cell interior counts as score 0
//     (cv::FAST zero-fills its score rows and never scores the 3 px frame of the Mat it is given);
//   * score = max(t, max_arc min(v-ring), max_arc min(ring-v)) - 1 over the 16 arcs of length 9.
//
// MI355X mapping (k_fast_rows).  The unit of work is a ROW GROUP: up to 8 horizontally adjacent cells of one cell row (<= 250 px of
// interior), one single-wave workgroup per item, persistent launch, 12 workgroups per CU (wide tiles of <= 40 rows: 12 800 bytes of LDS each = the
// item's tile + its list; narrow tiles 16 per CU).  With ~1 % corners a single 31x31 cell leaves a wave's lanes mostly idle after the first pass and
// pays the per-cell bookkeeping 6342 times per frame; measured on 32 frames of 1080p the first design (one wave per cell: 0.48 ms) became 0.24 ms in
// round 2 and 0.143 ms in round 5.
//   stage   the item's tile (interior + 3 px apron, <= 256 x 70 px) is fetched with 16-byte loads into registers while the PREVIOUS
//           item is processed, then written to LDS; the only HBM traffic of the kernel is this one read of each level
//   scan A  quick reject on the four compass points, 4 pixel columns x 8 rows per lane and block: the block's 14 tile rows, reduced to 6
//           bits so that four pixels fit one plain 32-bit ALU operation; the horizontal ring pixels come from the neighbouring lanes (DPP
//           wave shifts), the vertical differences are shared between the pixels three rows apart; on wide items a block loads and reduces
//           only its 8 new rows: the six it shares with the block above and their three difference pairs stay in registers (two sets that
//           swap roles, no moves; narrow items put their half-waves on different rows and share nothing); the masks of a block are byte-
//           transposed across lanes (a cluster of hits would otherwise keep one lane busy for 18 rounds) and their bits go to an LDS
//           list as codes (wave prefix sum of popcounts, one short bit loop per lane)
//   corners maybe pixels (decoded on dense lanes): the exact compass test picks the ONE polarity a pixel can still be a corner of, and
//           the corner-score network of that polarity (three-input min / max over the 16 arcs of 9) is the segment test: score >= t
//           decides, the score is kept.  Corners are compacted in place (score tile coordinates + score); the few pixels that pass both
//           compass tests without being a bright corner are re-queued at the list end for the dark test
//   tile    once every corner is scored the pixel tile is dead: its LDS is zeroed and becomes the dense score tile, in which every
//           cell owns its columns plus one zero separator column, so the 3x3 NMS needs no cell-boundary logic
//   NMS     over the corner list; survivors take consecutive slots of their ITEM (a wave-uniform running count).
// The list has a fixed capacity; when a block would overflow it the scan runs the corner passes on what it has and spills the scored
// corners to a per-wave area in global memory; they come back into the score tile before the NMS, which then walks the non-zero
// bytes of the tile instead of the list.  Saturated images stay correct and merely lose batching.  Work distribution, geometry table
// and LDS budget: see the kernel, hs_fast.h (the schedule) and hs_plan_fast.hip (the launch plan).
// Output: each ITEM owns a fixed slot range (the slots of its cells, contiguous; no global atomics), filled from its first slot upwards in NO
// particular order — every order-dependent decision downstream uses the (cell, y, x) key of the reference's candidate order:
//   cand[slot] = { y<<16 | x,  score<<24 | cell }   (coordinates relative to (16,16), as in vToDistributeKeys; cell = row-major cell index
//                                                    of the level); one 8-byte store per survivor, ~20 records = two cache lines per item
//   cell_count[image][first global cell of the item] = number of slots used (the entries of the item's other cells are not written).
// Bound (rounds 5-6): half by SIMD throughput and half by what ONE wave can issue, at 3 waves per SIMD — 12 single-wave workgroups per CU
// is what BOTH the LDS (12 800 bytes) and the registers (142 VGPRs) allow; t = 0.240 + 3.37 / n ms per 128 frames for n workgroups per CU, so occupancy is
// the lever and every added instruction costs.  VALU 0.87 per busy CU cycle of a mix-weighted ceiling ~1.1.  LDS: 49 % of the busy cycles active, 18.5 % in
// bank conflicts, 78 % of THOSE in the corner pass (tools/fast_lds_conflicts.sh: the 34 ds_read_u8 ring gathers of two candidates per lane at random tile
// positions — 2.0 conflict cycles per LDS instruction, the birthday rate of 32 lanes on 32 banks; that phase keeps the LDS busy 74 % of its time).  Wider
// reads do not help: gfx950 executes a ds_read_b32 / b64 at a byte-unaligned address ~6 x slower than an aligned one (tools/micro/lds_gather.hip: 7
// unaligned ds_read_b64 per ring 2 250 ns against 17 ds_read_u8 600 ns per wave-iteration at 12 waves per CU), and aligned chunks need two reads + a
// per-lane byte shift per ring row.  HBM bytes = P per frame, read once (measured 1.05-1.06 x).
#include "hs_internal.h"

// The workgroup is one wave: its LDS operations execute in program order, so a hand-off through LDS only needs the LDS queue
// drained (no s_barrier, and no vmcnt wait that would expose the latency of the next item's prefetch).
#define WAVE_LDS_FENCE() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

// append: lanes with `flag` get consecutive slots after `base` (wave-uniform); returns the lane's slot, advances base
__device__ __forceinline__ int wave_append(bool flag, int& base)
{
    const unsigned long long m = __ballot(flag);
    const int slot = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    base += (int)__popcll(m);
    return slot;
}

// Corner score of one polarity: cv::FAST's cornerScore<16> is max(t, max_arc min(v-ring), max_arc min(ring-v)) - 1; for a corner of one
// polarity the other polarity's term cannot exceed t (no 9-arc passes it) while its own term does, so score = max_arc min(d) - 1 with
// d[k] = v - ring[k] (dark) or ring[k] - v (bright), and the pixel IS a corner of that polarity exactly when max_arc min(d) > t.
// Three-input min / max: lo3[k] = min(d[k..k+2]), arc9[k] = min(lo3[k], lo3[k+3], lo3[k+6]), a max3 tree over the 16 arcs — 16 + 16 + 8.
// Round 5: the network runs on the RAW bytes.  min / max commute with subtracting a constant, so max_arc min(ring - v) = max_arc min(ring) - v,
// and the dark polarity is the bright one on complemented bytes: v - ring = (255 - ring) - (255 - v) = (ring ^ 0xFF) - (v ^ 0xFF).  With the per-lane
// mask m = 0 (bright) / 0xFF (dark) the 16 differences are 16 v_xor_b32 — a plain VOP2 op of the class this chip issues at up to 1.4-1.6 wave-
// instructions per cycle and CU — instead of the 16 v_mad_i32_i24 of round 3 (VOP3: 0.85; profiles/r04_valu_issue_rates.txt), and one subtraction at the end.
__device__ __forceinline__ int fast_corner_score3(const int (&r)[16], int v, bool bright)
{
    const int m = bright ? 0 : 0xFF;
    int d[16], lo3[16], arc[16];
#pragma unroll
    for (int k = 0; k < 16; k++) asm("v_xor_b32 %0, %1, %2" : "=v"(d[k]) : "v"(m), "v"(r[k]));   // as asm: the compiler turns r ^ m into a select of r and ~r & 0xFF
    // (as asm as well: left to itself the compiler shares min(d[k+1], d[k+2]) between neighbours and ends up with 32 two-input minima)
    auto min3 = [](int x, int y, int z) { int o; asm("v_min3_i32 %0, %1, %2, %3" : "=v"(o) : "v"(x), "v"(y), "v"(z)); return o; };
    auto max3 = [](int x, int y, int z) { int o; asm("v_max3_i32 %0, %1, %2, %3" : "=v"(o) : "v"(x), "v"(y), "v"(z)); return o; };
#pragma unroll
    for (int k = 0; k < 16; k++) lo3[k] = min3(d[k], d[(k + 1) & 15], d[(k + 2) & 15]);
#pragma unroll
    for (int k = 0; k < 16; k++) arc[k] = min3(lo3[k], lo3[(k + 3) & 15], lo3[(k + 6) & 15]);
    int m6[6];
#pragma unroll
    for (int k = 0; k < 5; k++) m6[k] = max3(arc[3 * k], arc[3 * k + 1], arc[3 * k + 2]);
    m6[5] = arc[15];
    return max(max3(m6[0], m6[1], m6[2]), max3(m6[3], m6[4], m6[5])) - (v ^ m) - 1;
}

// TWO candidates per lane (round 5): gfx950 has a packed three-input minimum / maximum, but only for f16 (v_pk_minimum3_f16 / v_pk_maximum3_f16).
// A byte b under the bit pattern 0x6400 | b IS the f16 number 1024 + b (exponent 2^10, mantissa step 1): exact, ordered like b, never a NaN or a
// denormal — so the score network above runs on (candidate A, candidate B) pairs of such halves with the same 40 instructions one candidate needed.
// P[k] = ring_A[k] | ring_B[k] << 16 (bytes); mx = polarity masks (0 / 0xFF per half, as in fast_corner_score3) | 0x64006400: one v_xor_b32 per
// ring position complements AND biases both halves.  Returns the two halves 0x6400 + max_arc min(ring ^ m).
__device__ __forceinline__ uint32_t fast_arc_max_pk(const uint32_t (&P)[16], uint32_t mx)
{
    uint32_t d[16], lo3[16], arc[16];
#pragma unroll
    for (int k = 0; k < 16; k++) asm("v_xor_b32 %0, %1, %2" : "=v"(d[k]) : "v"(mx), "v"(P[k]));
    auto min3 = [](uint32_t x, uint32_t y, uint32_t z) { uint32_t o; asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(o) : "v"(x), "v"(y), "v"(z)); return o; };
    auto max3 = [](uint32_t x, uint32_t y, uint32_t z) { uint32_t o; asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(o) : "v"(x), "v"(y), "v"(z)); return o; };
#pragma unroll
    for (int k = 0; k < 16; k++) lo3[k] = min3(d[k], d[(k + 1) & 15], d[(k + 2) & 15]);
#pragma unroll
    for (int k = 0; k < 16; k++) arc[k] = min3(lo3[k], lo3[(k + 3) & 15], lo3[(k + 6) & 15]);
    uint32_t m6[6];
#pragma unroll
    for (int k = 0; k < 5; k++) m6[k] = max3(arc[3 * k], arc[3 * k + 1], arc[3 * k + 2]);
    m6[5] = arc[15];
    const uint32_t a = max3(m6[0], m6[1], m6[2]);
    return max3(a, m6[3], max3(m6[4], m6[5], m6[5]));
}

typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ us2 as_us2(uint32_t x) { return __builtin_bit_cast(us2, x); }
__device__ __forceinline__ uint32_t as_u32(us2 x) { return __builtin_bit_cast(uint32_t, x); }
// bound_ctrl: the lane without a source (lane 0 / lane 63) reads 0 — a single v_mov_b32_dpp, no separate zero-initialisation of the result
// (those lanes' outer pixels are apron columns and are masked out of the scan anyway)
__device__ __forceinline__ uint32_t lane_from_below(uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x138, 0xF, 0xF, true); }  // wave_shr:1
__device__ __forceinline__ uint32_t lane_from_above(uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x130, 0xF, 0xF, true); }  // wave_shl:1

// Quick reject of 2 pixels held in the HIGH bytes of the two 16-bit fields (low bytes: anything).  Exact condition:
// (r0 or r8 darker than v-t) and (r4 or r12 darker), or the same for brighter.  Garbage in the low bytes can only add
// false positives: a true difference >= t+1 is >= 256t+1 in field units.  Returns non-zero fields for pixels that may be corners.
__device__ __forceinline__ us2 fr_pretest(us2 T, us2 C, us2 B, us2 L, us2 R, us2 t16)
{
    const us2 dk = __builtin_elementwise_max(__builtin_elementwise_min(T, B), __builtin_elementwise_min(L, R));
    const us2 br = __builtin_elementwise_min(__builtin_elementwise_max(T, B), __builtin_elementwise_max(L, R));
    const us2 z = __builtin_elementwise_max(__builtin_elementwise_sub_sat(C, dk), __builtin_elementwise_sub_sat(br, C));
    return __builtin_elementwise_sub_sat(z, t16);
}
// 1 in every 16-bit field that is non-zero (v_pk_min_u16; written as asm so that it is not turned back into compares)
__device__ __forceinline__ uint32_t fr_field_flags(us2 s, uint32_t ones)
{
    uint32_t r;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(as_u32(s)), "v"(ones));
    return r;
}

struct RowGeom {            // wave-uniform description of one work item in one image
    int img;
    int ncell, c0, gcell0;  // cells in this item, cell index of its first cell (within the level / within the image)
    uint32_t slot0; int ccap;
    int inv_w, inv_w1;
    int xoff, yoff;         // j0*wCell, i*hCell
    int th, ih, iw;         // tile rows, interior rows, interior width
    int off, ndw;           // tile column of level x is off + (x - iniX); dwords per tile row
    const uint8_t* rows;    // address of (a0, iniY): first dword of the first tile row
    size_t pitch;
    bool valid, aligned;
    int level;
};

// An item's record as ONE 64-byte scalar load.  Read field by field (`items[i]`) the compiler fetches the dword-sized fields with scalar loads and the
// byte / half-word ones (off, ndw, ...) with a VECTOR load whose round trip through L2 the wave then waits for — once per work item, on its critical path.
typedef uint32_t hs_u32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ HsFastItem fast_item_load(const HsFastItem* p) { return __builtin_bit_cast(HsFastItem, hs_cload<hs_u32x16>(p)); }
// the item's record (`items` already points at the launch's first item) + the image -> geometry
__device__ __forceinline__ RowGeom geom_of(const HsFastItem& it, const HsImg0& img0, int img)
{
    RowGeom g;
    g.img = img;
    g.ncell = it.ncell; g.c0 = it.c0; g.gcell0 = it.gcell0; g.slot0 = it.slot0; g.ccap = it.ccap;
    g.inv_w = it.inv_w; g.inv_w1 = it.inv_w1;
    g.xoff = it.xoff; g.yoff = it.yoff;
    g.th = it.th; g.ih = g.th - 6; g.iw = it.iw;
    g.off = it.off; g.ndw = it.ndw;
    g.valid = it.th != 0;
    g.level = it.level;
    const uint8_t* base;
    if (it.base == nullptr) { base = hs_img0_ptr(img0, g.img); g.pitch = img0.row_stride; }
    else { base = it.base + (size_t)g.img * it.img_stride; g.pitch = (size_t)it.pitch; }
    g.aligned = (((uintptr_t)base | g.pitch) & 3) == 0;
    g.rows = base + (size_t)it.iniY * g.pitch + it.a0;
    return g;
}
__device__ __forceinline__ RowGeom row_geom(const HsFastItem* __restrict__ items, const HsImg0& img0, int items_per_img, const FastSched& S, int w)
{
    int img;
    const int item = unit_decode(items_per_img, S, w, &img);
    return geom_of(fast_item_load(items + item), img0, img);
}

// One wave per workgroup: its LDS instructions execute in issue order, so a later read sees an earlier write without any wait;
// FR_FENCE marks the hand-over points (define it as WAVE_LDS_FENCE() to wait for the LDS queue there).
#ifndef FR_FENCE
#define FR_FENCE() do {} while (0)
#endif

// Instruction-budget builds (tools/fast_instr_breakdown.sh): make EXTRA=-DFR_STOP=n cuts the item short after phase n — 1 scan A masks,
// 2 + list expansion, 3 + segment test, 4 + scores; results are meaningless (no candidates come out), only the SQ counters are read.
#ifndef FR_STOP
#define FR_STOP 99
#endif
#if defined(HS_FAST_PROFILE) || defined(HS_FAST_WAVES)   // make EXTRA=-DHS_FAST_WAVES: two real-time stamps per item and nothing else (tools/fast_wave_timeline.py)
__device__ unsigned long long g_fr_wave[4096 * 16];          // per workgroup: first stamp, stamp after the first item, last stamp, items, longest item (10 ns ticks), its work index,
                                                             // level << 32 | corners of the FIRST item, then its phase stamps: tile staged, next item prefetched, scan A done, corners scored, NMS done
extern "C" void hs_debug_fast_waves(unsigned long long* out /*[4096 * 16]*/)
{
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fr_wave), sizeof(unsigned long long) * 4096 * 16);
}
#endif
#ifdef HS_FAST_PROFILE       // make EXTRA=-DHS_FAST_PROFILE: per-phase cycle totals over all waves (tools/fast_phase_profile.py)
__device__ unsigned long long g_fr_prof[16];
#define FR_T(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define FR_ACC(i, a, b) fr_acc[i] += (b) - (a)
extern "C" void hs_debug_fast_profile(unsigned long long* out16)
{
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_fr_prof), sizeof(unsigned long long) * 16);
    unsigned long long z[16] = {};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_fr_prof), z, sizeof(z));
}
#else
#define FR_T(var)
#define FR_ACC(i, a, b)
#endif
#if defined(HS_FAST_WAVES)
#define FR_W(i) do { if (fr_items == 0) fr_ph[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define FR_W(i) do {} while (0)
#endif

// TR = tile rows held in LDS (6 + 8*RS*blocks); the item's tile (th <= TR rows) is fetched with 16-byte loads, 64/LPR rows per load
// KEYS: the quadtree's geometric keys are produced by this launch (calls of <= 16 frames: hs_api.hip).  A template parameter, not a runtime
// flag: the large-batch instantiation pays neither registers nor instructions for a path it never runs (round 4 carried it as a runtime
// flag: 139 -> 147 VGPRs and +1 M wave-instructions per 32 frames for nothing).
// Launch bounds: the narrow instances of the standard tile heights run 16 workgroups per CU, which 4 waves per SIMD = 128 VGPRs must allow (the
// per-item list placement of round 5 took the keyed one to 132 without the hint: 12 per CU, +20 % at one pair per call); the others are bound by LDS.
template <int LC, int TR, bool KEYS>
__global__ __launch_bounds__(64, (LC == 5 && TR <= 44 ? 4 : 1)) void k_fast_rows(const HsFastItem* __restrict__ items, HsImg0 img0, int fast_th,
                                                  uint2* __restrict__ cand,
                                                  int32_t* __restrict__ cell_count, uint64_t cand_img_stride,
                                                  int total_cells, int items_per_img, int total_work, FastRowsLds lds, int force_scan_b,
                                                  uint32_t* __restrict__ overflow, uint32_t overflow_stride, uint32_t epoch, int item_first, uint32_t spill_base, FastSched S,
                                                  const HsFastQt* __restrict__ qt, uint32_t* __restrict__ qhist, unsigned long long* __restrict__ qbest,
                                                  uint32_t qhist_img_stride, uint32_t qbest_img_stride)
{
    constexpr int COLS = 1 << LC;            // dwords per tile row
    constexpr int RS = 64 / COLS;            // half-waves working on different rows in the scans
    constexpr int PITCH = 4 * COLS + FR_PAD; // bytes per row of the pixel tile and of the score tile (padded: vertical neighbours in different banks)
    constexpr int PD = PITCH / 4;
    constexpr int LPR = COLS / 4;            // lanes per tile row in the 16-byte staging loads
    constexpr int RPL = 64 / LPR;            // tile rows per staging load
    constexpr int NL = (TR + RPL - 1) / RPL; // staging loads per lane
    constexpr int BR = 8;                    // rows per lane and scan block
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t* const tile = smem;
    uint8_t* const score = smem;                                                 // the score tile REUSES the pixel tile once every corner is scored
    uint32_t* const cellcnt = reinterpret_cast<uint32_t*>(smem + lds.off_cnt);   // survivors per cell of the item
    uint32_t* const queue = overflow + (size_t)(epoch & 3) * HS_FAST_QUEUE_DWORDS;   // 8 work counters, 128 bytes apart
    if (blockIdx.x == 0 && threadIdx.x < HS_FAST_NQ_MAX) overflow[(size_t)((epoch + 2) & 3) * HS_FAST_QUEUE_DWORDS + threadIdx.x * 32] = 0u;
    uint32_t* const ovf = overflow + 4 * HS_FAST_QUEUE_DWORDS + spill_base + (size_t)blockIdx.x * overflow_stride;   // this wave's spill area for scored corners (list overflow only)
    const uint32_t* const tile32 = reinterpret_cast<const uint32_t*>(tile);
    const uint32_t* const score32 = reinterpret_cast<const uint32_t*>(score);

    items += item_first;                                         // this launch covers items [item_first, item_first + items_per_img) of every image
    const int tid = threadIdx.x;
    const int col = tid & (COLS - 1), sub = tid >> LC;
    const int ld_row = tid / LPR, ld_c16 = tid % LPR;
    const int t = min(max(fast_th, 0), 255);
    const uint32_t kbias = (0x80u - (uint32_t)((t + 1) >> 2)) * 0x01010101u;     // see scan A
    constexpr int RO[16] = { 3 * PITCH + 0, 3 * PITCH + 1, 2 * PITCH + 2, 1 * PITCH + 3, 0 * PITCH + 3, -1 * PITCH + 3, -2 * PITCH + 2, -3 * PITCH + 1,
                             -3 * PITCH + 0, -3 * PITCH - 1, -2 * PITCH - 2, -1 * PITCH - 3, 0 * PITCH - 3, 1 * PITCH - 3, 2 * PITCH - 2, 3 * PITCH - 1 };

    // Work distribution: the item list is cut into 8 contiguous ranges, one per queue (home queue = blockIdx % 8, i.e. the waves that share
    // an XCD under round-robin placement, so that neighbouring items — shared apron lines — meet in one L2; placement is a speed
    // matter only).  A wave takes its FIRST item statically (range start + its rank among the queue's waves) and every further item from
    // the queue's atomic counter: corner-rich items cost several times more than flat ones, and with static strides the slowest of the
    // 2816 waves (5 items each) set the kernel time while the average wave idled for a third of it (SQ counters: 68 % VALU issue, 27 % of
    // wave cycles waiting).  The grab for the item after next is issued right after the next tile's prefetch and consumed an item later,
    // so its latency is never exposed; 8 counters on lines of their own see ~11 grabs/us each.  When a queue runs dry its waves steal
    // from the other queues, and leave when all eight are empty (every wave reaches that exit: the counters only grow).
    // Four counter sets rotate between launches: a launch uses set `epoch & 3` and its first workgroup zeroes set `(epoch + 2) & 3` for the
    // launch after next — no memset launch in the chain.  Two consecutive launches of a handle may run CONCURRENTLY (level 0 beside the
    // pyramid, the other levels after it: hs_api.hip), which is why the set a launch zeroes is not the next launch's.
    const int nq = 1 << S.nq_log, per_x = S.per_q, wpx = gridDim.x >> S.nq_log;
    int q = (int)(blockIdx.x & (nq - 1));                        // current queue (wave-uniform); blockIdx % 8 = the XCD under round-robin placement
    auto q_size = [&](int qq) { return fast_queue_size(S, qq, total_work, items_per_img); };
    // one lane asks; the value comes back in a VGPR and is only read (readfirstlane) an item later
    auto grab_async = [&](int qq) -> uint32_t {
        uint32_t v = 0;
        if (tid == 0) v = atomicAdd(&queue[qq * 32], 1u);
        return v;
    };
    // raw counter value -> work unit, stealing from the other queues when the home queue is exhausted; -1 = nothing left anywhere.
    // A thief first LOOKS at all eight counters with one load (lanes 0..7; plain loads do not serialise like atomics) and only then grabs
    // from the fullest queue: at the end of a launch thousands of waves would otherwise queue up failing atomics on eight addresses.
    const bool fold = S.mode == 4;                               // folded static schedule: no counters at all
    int fold_next = -1;
    if (fold) { const int u2 = 2 * (int)gridDim.x - 1 - (int)blockIdx.x; if (u2 < total_work) fold_next = u2; }
    const bool dynamic = !fold && wpx < per_x;                   // fewer items than waves: the static first items are the whole job
    auto resolve = [&](uint32_t raw) -> int {
        if (fold) { const int r = fold_next; fold_next = -1; return r; }
        if (!dynamic) return -1;
        int idx = (int)__builtin_amdgcn_readfirstlane(raw) + wpx;
        if (idx < q_size(q)) return q * per_x + idx;
        for (int tries = 0; tries < 8; tries++) {
            int rem = 0;
            if (tid < nq) rem = q_size(tid) - wpx - (int)__hip_atomic_load(&queue[tid * 32], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int best = 0, best_q = -1;
            for (int i = 0; i < nq; i++) { const int r = __builtin_amdgcn_readlane(rem, i); if (r > best) { best = r; best_q = i; } }
            if (best_q < 0) return -1;
            q = best_q;
            idx = (int)__builtin_amdgcn_readfirstlane(grab_async(q)) + wpx;      // synchronous: only at the very end of the launch
            if (idx < q_size(q)) return q * per_x + idx;
        }
        return -1;
    };
    int w = fold ? ((int)blockIdx.x < total_work ? (int)blockIdx.x : -1)
                 : (int)(blockIdx.x >> S.nq_log) < q_size(q) ? q * per_x + (int)(blockIdx.x >> S.nq_log) : (dynamic ? resolve(grab_async(q)) : -1);
    if (w < 0) return;
    uint32_t raw_next = dynamic ? grab_async(q) : 0u;            // the second item

    if (tid < FR_MAXG) cellcnt[tid] = 0;

#ifdef HS_FAST_PROFILE
    unsigned long long fr_acc[10] = {};
    FR_T(t_kernel0);
#endif
#if defined(HS_FAST_PROFILE) || defined(HS_FAST_WAVES)
    const unsigned long long fr_real0 = __builtin_amdgcn_s_memrealtime();     // the 100 MHz real-time counter: the same on every CU (s_memtime is not)
    unsigned long long fr_prev = fr_real0, fr_first = 0, fr_long = 0, fr_long_w = 0, fr_items = 0;
    unsigned fr_codes = 0;
    unsigned long long fr_ph[6] = {};                         // first item: level << 32 | corners, phase stamps
#endif
    hs_u32x4 pre[NL];
    RowGeom g = row_geom(items, img0, items_per_img, S, w);
    // All NL loads are issued unconditionally (rows beyond the tile re-read its last row, columns beyond it the last needed
    // 16 bytes): predicating them makes the compiler copy the whole register array at every merge point.
    auto prefetch = [&](const RowGeom& q) {
        const int rlast = max(q.th - 1, 0);
        const uint32_t coff = 16u * (uint32_t)min(ld_c16, (q.ndw - 1) >> 2);
        const uint8_t* base = hs_uniform_ptr(q.rows);
        if (q.aligned) {
#pragma unroll
            for (int k = 0; k < NL; k++)
                pre[k] = hs_gload_off<hs_u32x4>(base, (uint32_t)min(RPL * k + ld_row, rlast) * (uint32_t)q.pitch + coff);
        } else {                                                 // caller's frame with an odd base or stride: unaligned dword loads
            struct __attribute__((packed, aligned(1))) U32 { uint32_t v; };
#pragma unroll
            for (int k = 0; k < NL; k++) {
                const HS_GLOBAL U32* p = (const HS_GLOBAL U32*)((const HS_GLOBAL uint8_t*)(uintptr_t)base + ((uint32_t)min(RPL * k + ld_row, rlast) * (uint32_t)q.pitch + coff));
                pre[k] = hs_u32x4{p[0].v, p[1].v, p[2].v, p[3].v};
            }
        }
    };
    prefetch(g);

    for (; w >= 0;) {
        int32_t* const cnt_out = &cell_count[(size_t)g.img * total_cells + g.gcell0];
        if (!g.valid) {
            if (tid == 0) cnt_out[0] = 0;
            w = resolve(raw_next);
            if (w >= 0) { g = row_geom(items, img0, items_per_img, S, w); prefetch(g); if (dynamic) raw_next = grab_async(q); }
            continue;
        }
        const RowGeom cur = g;
        // The next work unit: its queue counter value was requested an item ago and arrives with the tile loads the staging below waits for anyway;
        // its item record (one 64-byte scalar load) is requested BEFORE the staging stores, so that it is there when they are done.
        FR_T(t0);
        const int w_next = resolve(raw_next);
        int img_next = 0;
        const int item_next = w_next >= 0 ? unit_decode(items_per_img, S, w_next, &img_next) : 0;
        const HsFastItem it_next = fast_item_load(items + item_next);      // (no next unit: item 0's record, unused)
        // ---- stage the tile
#pragma unroll
        for (int k = 0; k < NL; k++)
            if (RPL * (k + 1) <= TR || RPL * k + ld_row < TR)
                *reinterpret_cast<hs_u32x4*>(&tile[(RPL * k + ld_row) * PITCH + 16 * ld_c16]) = pre[k];
        FR_FENCE();
        FR_T(t1);
        FR_ACC(0, t0, t1);
        FR_W(1);
        // the item's pixel list starts where its tile ends (rows th .. TR of the tile region are not used by this item)
        const int list_off = cur.th * PITCH;
        const int pcap = min(lds.pcap_max, (int)((((uint32_t)(lds.off_cnt - list_off) * 43691u) >> 17) & ~15u));      // floor(bytes / 3) entries, a multiple of 16
        uint16_t* const plist = reinterpret_cast<uint16_t*>(smem + list_off);        // pixel entries: row<<8 | column (| 0x8000)
        uint8_t* const pscore = smem + list_off + 2 * pcap;                          // score of corner i of the list
        const int inv_w = cur.inv_w, inv_w1 = cur.inv_w1;
        const size_t slot_base = (size_t)cur.img * cand_img_stride + cur.slot0;
        const RowGeom g_next = geom_of(it_next, img0, img_next);       // (unconditional: a use inside the branch would sink the record's load below the staging stores)
        if (w_next >= 0) { g = g_next; prefetch(g); if (dynamic) raw_next = grab_async(q); }   // the next tile: in flight during the passes
        FR_T(t2);
        FR_ACC(1, t1, t2);
        FR_W(2);

        // ---- the quadtree's geometric keys (round 4): a survivor's key is xkey[x] | ykey[y] (HsFastQt).  The item's slices of the two tables are
        //      fetched NOW into registers — lane j holds the keys of interior columns 2 j, 2 j + 1 (kx0) and 128 + 2 j, 129 + 2 j (kx1; wide tiles
        //      only) and of interior rows 2 j, 2 j + 1 (ky0; a cell has at most 125 rows) — and read per survivor with ds_bpermute at the very end
        //      of the item, so their latency is never exposed.  The survivors' key histogram and the best candidate per key go to global memory
        //      with fire-and-forget atomics: the quadtree kernel starts from them instead of gathering the candidates.
        uint32_t kx0 = 0, kx1 = 0, ky0 = 0;
        bool keys_on = false;
        uint32_t* khist = nullptr; unsigned long long* kbest = nullptr;
        if constexpr (KEYS) {
            typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
            const HsFastQt Q = __builtin_bit_cast(HsFastQt, hs_cload<u32x8>(qt + cur.level));      // one s_load_dwordx8
            keys_on = Q.enabled != 0;
            if (keys_on) {
                struct __attribute__((packed, aligned(2))) U32 { uint32_t v; };
                typedef const HS_GLOBAL U32* gu32;
                const uint8_t* xb = hs_uniform_ptr(reinterpret_cast<const uint8_t*>(Q.xkey + (cur.xoff + 3)));
                const uint8_t* yb = hs_uniform_ptr(reinterpret_cast<const uint8_t*>(Q.ykey + (cur.yoff + 3)));
                kx0 = ((gu32)((const HS_GLOBAL uint8_t*)(uintptr_t)xb + 4u * (uint32_t)tid))->v;
                if (COLS > 32) kx1 = ((gu32)((const HS_GLOBAL uint8_t*)(uintptr_t)xb + (256u + 4u * (uint32_t)tid)))->v;
                ky0 = ((gu32)((const HS_GLOBAL uint8_t*)(uintptr_t)yb + 4u * (uint32_t)tid))->v;
                khist = qhist + (size_t)cur.img * qhist_img_stride + Q.hist_off;
                kbest = qbest + (size_t)cur.img * qbest_img_stride + Q.best_off;
            }
        }
        const int c_first = cur.off + 3;                         // tile column of the first interior pixel
        uint32_t vmask8 = 0;                                     // this lane's pixels that are interior columns: byte j = pixel j, one bit per row of a scan block
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int px = 4 * col + j - c_first;
            if (px >= 0 && px < cur.iw) vmask8 |= 0xFFu << (8 * j);
        }
        int npx = 0;                                             // wave-uniform list length
        int n_done = 0, n_ovf = 0;                               // scored corners at the head of the list (entries [n_done, npx) are scan codes); corners spilled
        int n_emit = 0;                                          // survivors of the item so far (wave-uniform)

        // ---- pixel list -> corners -> scores
        // ---- scan codes [n_done, npx) of the list -> corners -> scores; the scored corners stay at the head of the list
        auto corners_and_scores = [&]() {
            if (FR_STOP <= 2) { npx = n_done = 0; return; }
            FR_FENCE();
            FR_T(tc0);
#if defined(HS_FAST_WAVES)
            const int fr_n0 = n_done;
#endif
            int n_corner = n_done;
            int nend = npx;                                  // list end including the re-queued pixels (below)
            // Two candidates per lane and iteration: A = entry i0 + lane, B = entry i0 + 64 + lane (neighbouring lanes keep neighbouring entries: the
            // ring reads of a wave-instruction stay spatially close).  Decoding, ring reads and the exact compass test are per candidate; the score
            // network — 40 of the ~110 instructions a candidate cost — serves both (fast_arc_max_pk).
            for (int i0 = n_done; i0 < nend; i0 += 128) {
                const int iA = i0 + tid, iB = iA + 64;
                const bool actA = iA < nend, actB = iB < nend;
                const int codeA = plist[actA ? iA : 0], codeB = plist[actB ? iB : 0];
                int pyA, pxA, pyB, pxB;
                auto decode = [&](int code, int& py, int& px) {
                    const int eb = code & 31, ew = (code >> 5) & 63;                 // bit of the scan mask (8 * pixel + row), lane that held the word
                    const int el = (ew & 48) | ((ew - ((code & 24) >> 1)) & 15);     // lane that found it: byte j sits 4 j lanes up in its row of 16
                    py = BR * (RS * ((code >> 11) & 15) + (el >> LC)) + (eb & 7);
                    px = 4 * (el & (COLS - 1)) + (eb >> 3) - c_first;
                };
                decode(codeA, pyA, pxA); decode(codeB, pyB, pxB);
                const bool redo_darkA = codeA & 0x8000, redo_darkB = codeB & 0x8000;   // re-queued: passed both compass tests and is no bright corner
                const uint8_t* ctrA = &tile[(pyA + 3) * PITCH + c_first + pxA];
                const uint8_t* ctrB = &tile[(pyB + 3) * PITCH + c_first + pxB];
                const int vA = ctrA[0], vB = ctrB[0];
                int rA[16], rB[16];
#pragma unroll
                for (int k = 0; k < 16; k++) { rA[k] = ctrA[RO[k]]; rB[k] = ctrB[RO[k]]; }
                // ONE polarity per pixel, and the corner SCORE as the segment test.  A 9-arc contains two adjacent compass points (ring 0, 4,
                // 8, 12), so a dark corner passes the exact compass test "(r0 or r8 darker) and (r4 or r12 darker)" and a bright corner its
                // mirror image; the pixel goes through the score network of the polarity that can still succeed: it is a corner of that
                // polarity exactly when max_arc min(d) > t, i.e. score >= t (cornerScore's own definition).
                const bool dark_okA = max(min(rA[0], rA[8]), min(rA[4], rA[12])) < vA - t, bright_okA = min(max(rA[0], rA[8]), max(rA[4], rA[12])) > vA + t;
                const bool dark_okB = max(min(rB[0], rB[8]), min(rB[4], rB[12])) < vB - t, bright_okB = min(max(rB[0], rB[8]), max(rB[4], rB[12])) > vB + t;
                const bool brightA = bright_okA && !redo_darkA, brightB = bright_okB && !redo_darkB;
                uint32_t P[16];
#pragma unroll
                for (int k = 0; k < 16; k++) P[k] = (uint32_t)rA[k] | ((uint32_t)rB[k] << 16);
                const int mA = brightA ? 0 : 0xFF, mB = brightB ? 0 : 0xFF;
                const uint32_t R = fast_arc_max_pk(P, 0x64006400u | (uint32_t)mA | ((uint32_t)mB << 16));
                int scA = (int)(R & 0x3FFu) - (vA ^ mA) - 1, scB = (int)((R >> 16) & 0x3FFu) - (vB ^ mB) - 1;
                bool cornerA = scA >= t && actA && (dark_okA || bright_okA), cornerB = scB >= t && actB && (dark_okB || bright_okB);
                // Pixels that pass BOTH compass tests (6-8 % of the candidates on the reduced levels, 0.1 % on level 0) and are no bright
                // corner need the dark test as well: they go back to the END of the list with bit 15 set and fill the lanes of the last,
                // partly empty iteration (running the second test in place would double the cost of nearly every iteration).  The last
                // iteration itself (whose lanes already cover the list end) and a full list run the second test in place.
                const bool redoA = actA && dark_okA && bright_okA && !cornerA && !redo_darkA, redoB = actB && dark_okB && bright_okB && !cornerB && !redo_darkB;
                if (__any(redoA || redoB)) {
                    if (i0 + 128 < nend && nend + 128 <= pcap) {
                        const int slotA = wave_append(redoA, nend);
                        if (redoA) plist[slotA] = (uint16_t)(codeA | 0x8000);
                        const int slotB = wave_append(redoB, nend);
                        if (redoB) plist[slotB] = (uint16_t)(codeB | 0x8000);
                    } else {
                        const uint32_t R2 = fast_arc_max_pk(P, 0x64FF64FFu);
                        const int s2A = (int)(R2 & 0x3FFu) - (vA ^ 0xFF) - 1, s2B = (int)((R2 >> 16) & 0x3FFu) - (vB ^ 0xFF) - 1;
                        if (redoA && s2A >= t) { cornerA = true; scA = s2A; }
                        if (redoB && s2B >= t) { cornerB = true; scB = s2B; }
                    }
                }
                FR_FENCE();                                // this iteration's reads precede the in-place compaction writes
                const int slotA = wave_append(cornerA, n_corner);
                if (cornerA) {
                    const int gc = (pxA * inv_w) >> 16;          // cell of the item; its columns start at 1 + gc*(wcell+1)
                    plist[slotA] = (uint16_t)(((pyA + 1) << 8) | (1 + pxA + gc));     // score tile coordinates: what nms_and_emit reads
                    pscore[slotA] = (uint8_t)scA;
                }
                const int slotB = wave_append(cornerB, n_corner);
                if (cornerB) {
                    const int gc = (pxB * inv_w) >> 16;
                    plist[slotB] = (uint16_t)(((pyB + 1) << 8) | (1 + pxB + gc));
                    pscore[slotB] = (uint8_t)scB;
                }
            }
            FR_FENCE();
            FR_T(tc1);
            FR_ACC(4, tc0, tc1);
            if (FR_STOP <= 4 && FR_STOP >= 3) { npx = n_done = 0; return; }
#if defined(HS_FAST_WAVES)
            if (fr_items == 0) fr_codes += (unsigned)(nend - fr_n0);
#endif
            npx = n_done = n_corner;
            FR_FENCE();
        };
        // the list is full of scored corners (saturated image): spill them (row, column, score) to this wave's global area
        auto spill_corners = [&]() {
            for (int i = tid; i < n_done; i += 64) ovf[n_ovf + i] = ((uint32_t)plist[i] << 8) | pscore[i];
            n_ovf += n_done;
            npx = n_done = 0;
        };
        // make room for `need` more scan codes: score what is pending (corners are ~1/3 of the codes); spill only if that is not enough
        auto make_room = [&](int need) {
            corners_and_scores();
            if (npx + need > pcap) spill_corners();
        };

        // ---- pixel list (score tile coordinates) -> strict 3x3 NMS -> the cells' slots, in no particular order (the quadtree kernel
        //      orders a cell's records by (y, x) when it gathers them)
        auto nms_and_emit = [&]() {
            FR_FENCE();
            for (int i0 = 0; i0 < npx; i0 += 64) {
                const int i = i0 + tid;
                const bool act = i < npx;
                const int pos = plist[act ? i : 0];
                const int r = pos >> 8, sc = pos & 255;
                const uint8_t* p = &score[r * PITCH + sc];
                const int s = p[0];
                // all eight neighbours are read before any is compared (&&-chains compile to eight dependent LDS round trips)
                const int n0 = p[-PITCH - 1], n1 = p[-PITCH], n2 = p[-PITCH + 1], n3 = p[-1], n4 = p[1], n5 = p[PITCH - 1], n6 = p[PITCH], n7 = p[PITCH + 1];
                const int nmax = max(max(max(n0, n1), max(n2, n3)), max(max(n4, n5), max(n6, n7)));
                const bool keep = act & (s > nmax);
                const int slot = wave_append(keep, n_emit);     // one running count per ITEM: its records are contiguous from slot0
                const int gc = ((sc - 1) * inv_w1) >> 16;
                const int px = sc - 1 - gc;                      // interior column within the item
                uint32_t gk = 0;
                if (KEYS && keys_on) {                           // (wave-uniform; every lane takes part in the permutes: inactive lanes read lane 0)
                    const int pxc = act ? px : 0, ryc = act ? r - 1 : 0;
                    uint32_t vx = (uint32_t)__builtin_amdgcn_ds_bpermute(((pxc & 127) >> 1) << 2, (int)kx0);
                    if (COLS > 32) { const uint32_t v1 = (uint32_t)__builtin_amdgcn_ds_bpermute(((pxc & 127) >> 1) << 2, (int)kx1); if (pxc >= 128) vx = v1; }
                    const uint32_t vy = (uint32_t)__builtin_amdgcn_ds_bpermute(((ryc & 127) >> 1) << 2, (int)ky0);
                    gk = ((vx >> (16 * (pxc & 1))) & 0xFFFFu) | ((vy >> (16 * (ryc & 1))) & 0xFFFFu);
                }
                if (keep) {
                    const uint32_t xy = ((uint32_t)(r - 1 + 3 + cur.yoff) << 16) | (uint32_t)(px + 3 + cur.xoff), sk = ((uint32_t)s << 24) | (uint32_t)(cur.c0 + gc);
                    cand[slot_base + (size_t)slot] = make_uint2(xy, sk);
                    if (KEYS && keys_on) {
                        // k_quadtree's `offer`: maximum response, first in (cell, y, x) order on ties (ORBExtractor.cpp:381-400)
                        const unsigned long long order = ((unsigned long long)(sk & 0xFFFFFFu) << 32) | xy;
                        const unsigned long long key = ((unsigned long long)(sk >> 24) << 56) | (0x00FFFFFFFFFFFFFFull - order);
                        __hip_atomic_fetch_add(&khist[gk >> 1], 1u << ((gk & 1) * 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_fetch_max(&kbest[gk], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
            npx = 0;
        };

        // ---- the set bits of M (one per pixel of this lane's scan block) -> pixel list.  SCORES: bit 4r+j, entries in score tile
        //      coordinates; otherwise bit 8j + r, entries relative to the interior.  `row0`: tile/score row of r = 0.
        // Scan A entries are CODES (block<<11 | lane<<5 | bit of M), decoded on dense lanes by corners_and_scores: the per-lane bit loop
        // below runs for as many rounds as the busiest lane has hits, so every instruction in it counts ~10x.
        auto emit_mask = [&](uint32_t M, int row0, bool scores, int blk) {
            const uint32_t code0 = ((uint32_t)blk << 11) | ((uint32_t)tid << 5);
            const int incl = wave_scan_incl((int)__popc(M));
            const int total = __builtin_amdgcn_readlane(incl, 63);
            if (total == 0) return;
            if (npx + total > pcap) { if (scores) nms_and_emit(); else make_room(min(total, pcap)); }
            if (total <= pcap) {
                int pos = npx + incl - (int)__popc(M);
                while (M) {
                    const int b = __ffs((int)M) - 1;
                    M &= M - 1;
                    plist[pos++] = scores ? (uint16_t)(((row0 + (b >> 2)) << 8) | (4 * col + (b & 3))) : (uint16_t)(code0 | (uint32_t)b);
                }
                npx += total;
            } else {                                             // a block alone overflows the list (saturated image): one row at a time
                for (int r = 0; r < BR; r++) {
                    uint32_t Mr = M & (scores ? (0xFu << (4 * r)) : (0x01010101u << r));
                    const int incl_r = wave_scan_incl((int)__popc(Mr));
                    const int total_r = __builtin_amdgcn_readlane(incl_r, 63);      // <= 256 <= pcap
                    if (npx + total_r > pcap) { if (scores) nms_and_emit(); else make_room(total_r); }
                    int pos = npx + incl_r - (int)__popc(Mr);
                    while (Mr) {
                        const int b = __ffs((int)Mr) - 1;
                        Mr &= Mr - 1;
                        plist[pos++] = scores ? (uint16_t)(((row0 + r) << 8) | (4 * col + (b & 3))) : (uint16_t)(code0 | (uint32_t)b);
                    }
                    npx += total_r;
                }
            }
        };

        // ---- scan A: quick reject.  A lane takes 4 pixel columns x 8 rows per block: 14 tile rows (wide items: the 8 the block above has not
        //      already reduced), the horizontal ring pixels from the neighbouring lanes (DPP wave shifts), four pixels per 32-bit operation.
        FR_T(t3);
        {
            const int yend = 3 + cur.ih;
            const int nblock = (cur.ih + BR * RS - 1) / (BR * RS);               // uniform trip count (the half-waves take different rows)
            // Four pixels per 32-bit operation: every byte holds a pixel reduced to 6 bits (q = v >> 2), which leaves two guard bits per
            // byte, so byte-wise differences never borrow across bytes.  With bias = 0x80 - k per byte, bit 7 of (q_a + bias - q_b) is
            // set exactly when q_a - q_b >= k (the byte stays within [0x80 - k - 0x3F, 0x80 - k + 0x3F]).  With k = (t + 1) / 4, "b darker than a by more than t" implies q_a - q_b >= k (floor((a - m) / 4)
            // <= floor(a / 4) - floor(m / 4)), so the byte test is a NECESSARY condition for the exact compass test of the 16-bit version it
            // replaces (measured: 3.7 % of the pixels pass instead of 3.6 %); the segment test on the full bytes follows as before.
            // ~26 plain 32-bit ALU operations per row of 4 pixels instead of ~34 packed-16-bit ones, which also issue slower.
            auto reduce6 = [&](const uint32_t* tp, int k) { return (tp[k * PD] >> 2) & 0x3F3F3F3Fu; };
            // The block's mask from its centre rows QC / GC (tile rows 3 .. 10 of the block) and its 11 vertical differences.
            // "x darker than C": bit 7 of (q_C + bias) - q_x; "x brighter": bit 7 of q_x + (bias - q_C).  Vertically the four differences
            // of a pixel are shared with the pixels three rows above and below it: with D1[y] = G[y] - Q[y+3] and D2[y] = G[y+3] - Q[y],
            // row c sees "top or bottom darker" = D2[c-3] | D1[c] and "top or bottom brighter" = D1[c-3] | D2[c] — two subtractions per
            // tile row instead of four per centre row (the same 32-bit values as the direct form, so the masks are the same bits).
            auto block_mask = [&](const uint32_t* QC, const uint32_t* GC, const uint32_t* D1, const uint32_t* D2, int y0) -> uint32_t {
                uint32_t M = 0;
#pragma unroll
                for (int r = 0; r < BR; r++) {
                    const uint32_t qC = QC[r];
                    const uint32_t gC = GC[r], nC = kbias - qC;
                    const uint32_t qCm = lane_from_below(qC), qCp = lane_from_above(qC);
                    const uint32_t qL = __builtin_amdgcn_alignbyte(qC, qCm, 1);          // the pixels 3 columns to the left / right of this lane's four
                    const uint32_t qR = __builtin_amdgcn_alignbyte(qCp, qC, 3);
                    const uint32_t dark = (D2[r] | D1[r + 3]) & ((gC - qL) | (gC - qR));           // (top or bottom darker) and (left or right darker)
                    const uint32_t bright = (D1[r] | D2[r + 3]) & ((qL + nC) | (qR + nC));
                    M = (M >> 1) | ((dark | bright) & 0x80808080u);                      // row r ends up at bit r of its pixel's byte
                }
                const int nrow = min(max(yend - y0, 0), BR);                     // rows of this block inside the interior
                M &= vmask8 & (((1u << nrow) - 1u) * 0x01010101u);
                // The maybe-pixels come in clusters (both sides of a slanted edge): on the bench scene a block has its ~120 hits in ~14 of
                // its 64 lanes, and the bit loop of emit_mask runs as long as the busiest lane has hits (17.7 rounds on average).  Each lane
                // therefore keeps byte 0 (its first pixel column) and takes byte j from the lane 4 j to its left in its row of 16 lanes (DPP
                // row rotate): the four columns of a lane's word are 16 px apart and a cluster's columns land in different lanes (9.3
                // rounds; 8.4 with the lanes 16 j apart, but then neighbouring list entries come from areas 64 px apart and the ring reads
                // of the segment test collide in the LDS banks).  corners_and_scores undoes it when it decodes a code.
                const uint32_t t1 = (uint32_t)__builtin_amdgcn_mov_dpp((int)M, 0x124, 0xF, 0xF, false), t2 = (uint32_t)__builtin_amdgcn_mov_dpp((int)M, 0x128, 0xF, 0xF, false),
                               t3 = (uint32_t)__builtin_amdgcn_mov_dpp((int)M, 0x12C, 0xF, 0xF, false);      // row_ror:4 / 8 / 12
                return (M & 0xFFu) | (t1 & 0xFF00u) | (t2 & 0xFF0000u) | (t3 & 0xFF000000u);
            };
            if constexpr (RS == 1) {
                // Consecutive blocks of a lane start 8 tile rows apart, so tile rows 8 .. 13 of a block are rows 0 .. 5 of the next one and its
                // differences D1 / D2[8 .. 10] are the next one's D1 / D2[0 .. 2].  What the next block still needs of them is CARRIED in registers
                // (rows 3 .. 5 reduced and biased, the three difference pairs; rows 0 .. 2 themselves only ever enter D2[0 .. 2]): a block loads and
                // reduces its 8 new rows and forms its 8 new difference pairs.  The item's first block takes its carry from a prologue over tile
                // rows 0 .. 5 — what it would have computed anyway — so carried state never crosses items.  Valid because nothing writes the pixel
                // tile during the scan (corners_and_scores reads it; list and scores start at row th), and because a block that runs has y0 < 3 + ih,
                // so its rows 0 .. 5 lie below row th: list memory (rows >= th, rewritten between blocks) is only ever read as a block's NEW rows,
                // exactly as before, and only reaches centre rows that the nrow mask removes.
                // Two register sets swap roles from block to block (the loop below is unrolled by two: even steps read ca and write cb, odd ones the
                // reverse), so the carry costs no register moves.  Only the usual hand-over of a block's codes — they fit the list — is part of that
                // loop (emit_codes); a block whose codes need room first leaves it with its mask, goes through emit_mask (the one copy of the
                // corner pass, which the carried values are NOT live across: the kernel's register peak is there) and the scan resumes behind it
                // from a fresh prologue.
                struct ScanCarry { uint32_t q[3], g[3], d1[3], d2[3]; };
                auto carried_block = [&](const ScanCarry& in, ScanCarry& out, int y0) -> uint32_t {
                    const uint32_t* tp = tile32 + (y0 - 3) * PD + col;
                    uint32_t Q[BR + 3], G[BR + 3];                                   // tile rows 3 .. 13 of the block
                    uint32_t D1[BR + 3], D2[BR + 3];
#pragma unroll
                    for (int k = 0; k < 3; k++) { Q[k] = in.q[k]; G[k] = in.g[k]; D1[k] = in.d1[k]; D2[k] = in.d2[k]; }
#pragma unroll
                    for (int k = 3; k < BR + 3; k++) { Q[k] = reduce6(tp, k + 3); G[k] = Q[k] + kbias; }
#pragma unroll
                    for (int y = 3; y < BR + 3; y++) { D1[y] = G[y - 3] - Q[y]; D2[y] = G[y] - Q[y - 3]; }
#pragma unroll
                    for (int k = 0; k < 3; k++) { out.q[k] = Q[BR + k]; out.g[k] = G[BR + k]; out.d1[k] = D1[BR + k]; out.d2[k] = D2[BR + k]; }
                    return block_mask(Q, G, D1, D2, y0);
                };
                // the usual case of emit_mask: the block's codes fit the list as it is.  false: nothing was written, the block needs emit_mask
                auto emit_codes = [&](uint32_t M, int blk) -> bool {
                    const int incl = wave_scan_incl((int)__popc(M));
                    const int total = __builtin_amdgcn_readlane(incl, 63);
                    if (npx + total > pcap) return false;
                    const uint32_t code0 = ((uint32_t)blk << 11) | ((uint32_t)tid << 5);
                    int pos = npx + incl - (int)__popc(M);
                    while (M) {
                        const int bit = __ffs((int)M) - 1;
                        M &= M - 1;
                        plist[pos++] = (uint16_t)(code0 | (uint32_t)bit);
                    }
                    npx += total;
                    return true;
                };
                for (int b = 0; b < nblock; b++) {
                    ScanCarry ca, cb;
                    {                                                                // the carry into block b from its tile rows 0 .. 5
                        const uint32_t* tp = tile32 + BR * b * PD + col;
                        uint32_t Q[6], G[6];
#pragma unroll
                        for (int k = 0; k < 6; k++) { Q[k] = reduce6(tp, k); G[k] = Q[k] + kbias; }
#pragma unroll
                        for (int k = 0; k < 3; k++) { ca.q[k] = Q[k + 3]; ca.g[k] = G[k + 3]; ca.d1[k] = G[k] - Q[k + 3]; ca.d2[k] = G[k + 3] - Q[k]; }
                    }
                    uint32_t M;
                    for (;;) {
                        M = carried_block(ca, cb, 3 + BR * b);
                        if (FR_STOP <= 1) { if (M == 0x12345u) plist[tid] = 1; }     // keeps M live
                        else if (!emit_codes(M, b)) break;
                        if (++b >= nblock) break;
                        M = carried_block(cb, ca, 3 + BR * b);
                        if (FR_STOP <= 1) { if (M == 0x12345u) plist[tid] = 1; }
                        else if (!emit_codes(M, b)) break;
                        if (++b >= nblock) break;
                    }
                    if (b < nblock) emit_mask(M, 3 + BR * b, false, b);
                }
            } else {
                // half-waves on different rows: a lane's consecutive blocks are 16 rows apart and share nothing (the scan as it was)
                for (int b = 0; b < nblock; b++) {
                    const int y0 = 3 + BR * (RS * b + sub);
                    uint32_t M = 0;
                    {
                        const uint32_t* tp = tile32 + (y0 - 3) * PD + col;
                        uint32_t Q[BR + 6], G[BR + 6];
#pragma unroll
                        for (int k = 0; k < BR + 6; k++) { Q[k] = (tp[k * PD] >> 2) & 0x3F3F3F3Fu; G[k] = Q[k] + kbias; }
                        uint32_t D1[BR + 3], D2[BR + 3];
#pragma unroll
                        for (int y = 0; y < BR + 3; y++) { D1[y] = G[y] - Q[y + 3]; D2[y] = G[y + 3] - Q[y]; }
#pragma unroll
                        for (int r = 0; r < BR; r++) {
                            const uint32_t qC = Q[r + 3];
                            const uint32_t gC = G[r + 3], nC = kbias - qC;
                            const uint32_t qCm = lane_from_below(qC), qCp = lane_from_above(qC);
                            const uint32_t qL = __builtin_amdgcn_alignbyte(qC, qCm, 1);          // the pixels 3 columns to the left / right of this lane's four
                            const uint32_t qR = __builtin_amdgcn_alignbyte(qCp, qC, 3);
                            const uint32_t dark = (D2[r] | D1[r + 3]) & ((gC - qL) | (gC - qR));           // (top or bottom darker) and (left or right darker)
                            const uint32_t bright = (D1[r] | D2[r + 3]) & ((qL + nC) | (qR + nC));
                            M = (M >> 1) | ((dark | bright) & 0x80808080u);                      // row r ends up at bit r of its pixel's byte
                        }
                        const int nrow = min(max(yend - y0, 0), BR);                     // rows of this block inside the interior
                        M &= vmask8 & (((1u << nrow) - 1u) * 0x01010101u);
                    }
                    {
                        const uint32_t t1 = (uint32_t)__builtin_amdgcn_mov_dpp((int)M, 0x124, 0xF, 0xF, false), t2 = (uint32_t)__builtin_amdgcn_mov_dpp((int)M, 0x128, 0xF, 0xF, false),
                                       t3 = (uint32_t)__builtin_amdgcn_mov_dpp((int)M, 0x12C, 0xF, 0xF, false);      // row_ror:4 / 8 / 12
                        M = (M & 0xFFu) | (t1 & 0xFF00u) | (t2 & 0xFF0000u) | (t3 & 0xFF000000u);
                    }
                    if (FR_STOP <= 1) { if (M == 0x12345u) plist[tid] = 1; continue; }      // keeps M live
                    emit_mask(M, y0, false, b);
                }
            }
            FR_W(3);
            corners_and_scores();
            FR_W(4);
        }
        FR_T(t4);
        FR_ACC(2, t3, t4);                                       // scan A including corners_and_scores (4, 5 are subsets)
        if (FR_STOP <= 4) n_done = 0;
        // ---- the pixel tile is dead: its LDS becomes the dense score tile (rows 0..ih+1, zero except at the corners)
        if (FR_STOP > 4) {
            if constexpr (TR <= 54) {                            // rows 0 .. ih+1 = th-5 in chunks of 1 KB at compile-time offsets; never into the list, which starts at
                const int zbytes = (cur.ih + 2) * PITCH;         // row th and is live here (wide tiles: a chunk is shorter than the four rows in between)
#pragma unroll
                for (int k = 0; k < ((TR - 4) * PITCH + 1023) / 1024; k++) {
                    if constexpr (4 * PITCH >= 1024) { if (1024 * k < zbytes) *reinterpret_cast<uint4*>(score + 1024 * k + 16 * tid) = make_uint4(0, 0, 0, 0); }          // wave-uniform test
                    else { if (1024 * k + 16 * tid < zbytes) *reinterpret_cast<uint4*>(score + 1024 * k + 16 * tid) = make_uint4(0, 0, 0, 0); }                          // narrow tiles: four rows are less than a chunk
                }
            } else {
                for (int i = tid * 16; i < (cur.ih + 2) * PITCH; i += 64 * 16) *reinterpret_cast<uint4*>(score + i) = make_uint4(0, 0, 0, 0);
            }
        }
        for (int i = tid; i < n_done; i += 64) {
            const int pos = plist[i];
            score[(pos >> 8) * PITCH + (pos & 255)] = pscore[i];
        }
        if (n_ovf > 0) {                                         // spilled corners come back through L2 (the wave's own stores: wait, then bypass L1)
            __builtin_amdgcn_s_waitcnt(0x0f70);                  // vmcnt(0)
            for (int i = tid; i < n_ovf; i += 64) {
                const uint32_t rec = __hip_atomic_load(&ovf[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                score[(rec >> 16) * PITCH + ((rec >> 8) & 255)] = (uint8_t)rec;
            }
        }
        // ---- NMS.  Usual case: every corner of the item is still in the list (score coordinates).
        if (n_ovf == 0 && !force_scan_b) {
            npx = n_done;
            nms_and_emit();
        } else {
            // ---- scan B (the list overflowed and corners were spilled): find the corners again as the non-zero bytes of the score tile
            FR_FENCE();
            npx = 0;                                             // the list is scratch from here on (its corners are in the tile)
            const int nblock = (cur.ih + BR * RS - 1) / (BR * RS);
            for (int b = 0; b < nblock; b++) {
                const int r0 = 1 + BR * (RS * b + sub);
                uint32_t M = 0;
#pragma unroll
                for (int r = 0; r < BR; r++) {
                    const uint32_t S = (r0 + r <= cur.ih) ? score32[(r0 + r) * PD + col] : 0u;
                    const uint32_t nib = ((S & 0xFFu) ? 1u : 0u) | ((S & 0xFF00u) ? 2u : 0u) | ((S & 0xFF0000u) ? 4u : 0u) | ((S & 0xFF000000u) ? 8u : 0u);
                    M |= nib << (4 * r);
                }
                emit_mask(M, r0, true, b);
            }
            if (npx > 0) nms_and_emit();
        }
        FR_FENCE();
        FR_T(t5);
        FR_ACC(6, t4, t5);
        // ---- the item's count (kept at its first cell's entry); reset the counter
        if (tid == 0) cnt_out[0] = (int32_t)n_emit;
        FR_FENCE();
        if (tid < FR_MAXG) cellcnt[tid] = 0;
#ifdef HS_FAST_PROFILE
        FR_FENCE();
        FR_T(t6);
        FR_ACC(7, t5, t6);
        fr_acc[8] += 1;
        fr_acc[3] += n_ovf > 0;
#endif
#if defined(HS_FAST_PROFILE) || defined(HS_FAST_WAVES)
        {
            const unsigned long long now = __builtin_amdgcn_s_memrealtime();
            if (fr_items == 0) { fr_first = now;
#if defined(HS_FAST_WAVES)
                fr_ph[0] = ((unsigned long long)(unsigned)cur.level << 32) | ((unsigned long long)(fr_codes & 0xFFFFu) << 16) | (unsigned)(n_done & 0xFFFF); fr_ph[5] = now;
#endif
            }
            if (now - fr_prev > fr_long) { fr_long = now - fr_prev; fr_long_w = (unsigned long long)(unsigned)w | ((unsigned long long)(n_ovf > 0) << 32); }
            fr_prev = now; fr_items++;
        }
#endif
        w = w_next;
    }
#ifdef HS_FAST_PROFILE
    FR_T(t_kernel1);
    fr_acc[9] = t_kernel1 - t_kernel0;
    if (tid == 0) for (int i = 0; i < 10; i++) atomicAdd(&g_fr_prof[i], fr_acc[i]);
    if (tid == 0) atomicAdd(&g_fr_prof[10], 1ull);
#endif
#if defined(HS_FAST_PROFILE) || defined(HS_FAST_WAVES)
    if (tid == 0 && blockIdx.x < 4096) {
        unsigned long long* o = &g_fr_wave[blockIdx.x * 16];
        o[0] = fr_real0; o[1] = fr_first; o[2] = __builtin_amdgcn_s_memrealtime(); o[3] = fr_items; o[4] = fr_long; o[5] = fr_long_w;
#if defined(HS_FAST_WAVES)
        for (int i = 0; i < 6; i++) o[8 + i] = fr_ph[i];
#endif
    }
#endif
}

// The launch: everything it decides is in the record (hs_fast_launch_plan, hs_plan_fast.hip); here it only picks the instance.
bool hs_launch_fast(const HsFastLaunch& P, const HsFastItem* d_items, HsImg0 img0, int fast_th, uint2* cand, int32_t* cell_count, uint64_t cand_img_stride, int total_cells,
                    uint32_t* overflow, uint32_t epoch, const HsFastQt* d_qt, uint32_t* qhist, unsigned long long* qbest, uint32_t qhist_img_stride, uint32_t qbest_img_stride, hipStream_t s)
{
    if (total_cells <= 0 || P.total_work <= 0) return false;
#define FR_LAUNCH_K(LC_, TR_, K_) hipLaunchKernelGGL((k_fast_rows<LC_, TR_, K_>), dim3(P.nblk), dim3(64), P.lds.total, s, d_items, img0, fast_th, cand, \
                                               cell_count, cand_img_stride, total_cells, P.items_per_img, P.total_work, P.lds, P.force_scan_b, overflow, P.ovf_stride, epoch, P.item_first, P.spill_base, P.S, \
                                               d_qt, qhist, qbest, qhist_img_stride, qbest_img_stride)
#define FR_LAUNCH(LC_, TR_) if (P.tr == TR_) { if (d_qt != nullptr) FR_LAUNCH_K(LC_, TR_, true); else FR_LAUNCH_K(LC_, TR_, false); }
#define FR_WIDE(TR_) FR_LAUNCH(6, TR_)
#define FR_NARROW(TR_) FR_LAUNCH(5, TR_)
    if (P.lc == 6) { HS_FAST_TILE_ROWS(FR_WIDE) } else { HS_FAST_TILE_ROWS(FR_NARROW) }
#undef FR_NARROW
#undef FR_WIDE
#undef FR_LAUNCH
#undef FR_LAUNCH_K
    return true;
}
