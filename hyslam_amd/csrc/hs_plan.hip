// hs_plan.hip — the extractor's configuration for one frame size as a pure host computation (HsPlan, hs_plan.h): level sizes and cell grid,
// cv::resize's fixed-point tables, the quadtree's key tables, the pyramid's fusion / chain / small-batch plans (hs_plan_pyramid.hip), both FAST
// work-item lists (hs_plan_fast.hip) and every per-image size.  No HIP call, no handle: pointer fields hold byte offsets until hs_api.hip has allocated the buffers they point into.
#include "hs_plan.h"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

namespace {

inline int cv_round_f(float v) { return (int)nearbyintf(v); }           // cvRound: round half to even
inline int cv_floor_f(float v) { int i = (int)v; return i - (i > v); }
inline short sat_short(float v) { int i = cv_round_f(v); return (short)(i < -32768 ? -32768 : (i > 32767 ? 32767 : i)); }

template <class T> T* at_offset(size_t bytes) { return reinterpret_cast<T*>((uintptr_t)bytes); }

struct Refusal { int code; const char* text; };
const Refusal OK{ HS_OK, "" };

// Level sizes (ORBExtractor.cpp:568-569), the FAST cell grid (:413-428), the wide work items, the quadtree's inputs (:183-185) and each level's
// place in one image's pyramid, candidate and selection arrays
Refusal plan_levels(const HsPlanInput& in, HsPlan& P)
{
    const int L = in.p->nlevels;
    P.lv.assign(L, HsLevel{});
    size_t pyr_per_img = 0; uint64_t cand = 0; int sel = 0, cells = 0, items = 0;
    for (int l = 0; l < L; l++) {
        HsLevel& V = P.lv[l];
        V.w = cv_round_f((float)in.w * in.inv_scale[l]);          // ORBExtractor.cpp:568-569
        V.h = cv_round_f((float)in.h * in.inv_scale[l]);
        if (V.w < 1 || V.h < 1) return { HS_ERR_INVALID, "pyramid level collapses to zero size" };
        V.pitch = (V.w + 63) & ~63;
        if (l > 0) { V.base = at_offset<uint8_t>(pyr_per_img); pyr_per_img += (size_t)V.pitch * V.h; }      // (level 1 at offset 0; level 0 is the caller's frame: nullptr)
        // cell grid, ORBExtractor.cpp:413-428
        const int minB = HS_BORDER, maxBX = V.w - HS_BORDER, maxBY = V.h - HS_BORDER;
        const float width = (float)(maxBX - minB), height = (float)(maxBY - minB);
        const float W = (float)in.p->cell_px;
        V.ncols = width > 0 ? (int)(width / W) : 0;
        V.nrows = height > 0 ? (int)(height / W) : 0;
        if (V.ncols < 1 || V.nrows < 1) { V.ncols = V.nrows = 0; V.wcell = V.hcell = 0; }   // reference: division by zero (UB); no keypoints here
        else { V.wcell = (int)ceilf(width / V.ncols); V.hcell = (int)ceilf(height / V.nrows); }
        if (V.wcell > hs_fast_max_cell_w(6) || V.hcell > HS_MAX_CELL_H)
            return { HS_ERR_INVALID, "FAST cell wider than 247 px or taller than 125 px is not supported" };
        V.cell_begin = cells; cells += V.ncols * V.nrows;
        V.grp_cells = hs_fast_group_cells(V.wcell, V.ncols, 6);
        V.ngroups = V.grp_cells > 0 ? (V.ncols + V.grp_cells - 1) / V.grp_cells : 0;
        V.item_begin = items; items += V.ngroups * V.nrows;
        V.inv_wcell = V.wcell > 0 ? (65536 + V.wcell - 1) / V.wcell : 0;
        V.inv_wcell1 = V.wcell > 0 ? (65536 + V.wcell) / (V.wcell + 1) : 0;
        // quadtree, ORBExtractor.cpp:183-185
        V.qt_w = maxBX - minB; V.qt_h = maxBY - minB;
        V.n_ini = (V.qt_w > 0 && V.qt_h > 0) ? (int)roundf((float)V.qt_w / (float)V.qt_h) : 0;
        if (V.ncols > 0 && V.n_ini < 1) return { HS_ERR_INVALID, "aspect ratio w/h < 0.5 is undefined behaviour in the reference (nIni == 0)" };
        if (V.ncols < 1) V.n_ini = 0;      // a level without a FAST cell has no keypoints (D4) and no tree: its aspect ratio refuses nothing (until round 6 a 560 x 33 level 7 did: 528 roots)
        if (V.n_ini > (in.qt_large ? HS_QT_LARGE_NODES : HS_QT_MAX_NODES) / 4) return { HS_ERR_INVALID, "aspect ratio too wide" };
        V.hx = V.n_ini > 0 ? (float)V.qt_w / V.n_ini : 1.f;
        V.quota = in.quota[l];
        V.cand_cap = V.ncols * V.nrows * hs_cell_cap(V.wcell, V.hcell);
        V.cand_off = cand; cand += (uint64_t)((V.cand_cap + 3) & ~3);
        V.sel_cap = std::max(V.quota + 4, 4 * V.n_ini + 4);
        V.sel_off = sel; sel += V.sel_cap;
        V.scale = in.scale[l];
        V.kp_size = (float)(int)(31 * in.scale[l]);              // ORBExtractor.cpp:478
    }
    P.pyr_per_img = hs_up256(pyr_per_img);
    for (int l = 0; l < L; l++) {
        P.lv[l].img_stride = P.pyr_per_img;
        P.max_wcell = std::max(P.max_wcell, P.lv[l].wcell); P.max_hcell = std::max(P.max_hcell, P.lv[l].hcell);
    }
    P.w = in.w; P.h = in.h;
    P.total_cells = cells; P.fast_items = items; P.cand_img_stride = cand; P.sel_img_stride = sel; P.max_kp = sel;
    return OK;
}

// cv::resize tables (OpenCV 3.4 resize.cpp, INTER_LINEAR, 8U fixed point) of every level l >= 1 from level l - 1
void plan_resize_tables(HsPlan& P)
{
    std::vector<int16_t>& tables = P.tables;
    for (size_t l = 1; l < P.lv.size(); l++) {
        HsLevel& V = P.lv[l];
        const int sw = P.lv[l - 1].w, sh = P.lv[l - 1].h;
        const double scale_x = 1. / ((double)V.w / sw), scale_y = 1. / ((double)V.h / sh);
        int xmax = V.w;
        auto grow = [&](size_t n) { size_t o = (tables.size() + 3) & ~(size_t)3; tables.resize(o + n); return o; };   // 8-byte aligned
        const size_t o0 = grow(4 * (size_t)V.w);   // x table: {sx, a0, a1, 0} per output column (xofs and ialpha are the same table)
        const size_t o2 = grow(V.h);               // yofs
        const size_t o3 = grow(2 * (size_t)V.h);   // ibeta
        for (int dx = 0; dx < V.w; dx++) {
            float fx = (float)((dx + 0.5) * scale_x - 0.5);
            int sx = cv_floor_f(fx); fx -= sx;
            if (sx < 0) { fx = 0; sx = 0; }
            if (sx + 1 >= sw) { xmax = std::min(xmax, dx); if (sx >= sw - 1) { fx = 0; sx = sw - 1; } }
            tables[o0 + 4 * dx] = (int16_t)sx;
            tables[o0 + 4 * dx + 1] = sat_short((1.f - fx) * 2048);
            tables[o0 + 4 * dx + 2] = sat_short(fx * 2048);
            tables[o0 + 4 * dx + 3] = 0;
        }
        for (int dy = 0; dy < V.h; dy++) {
            float fy = (float)((dy + 0.5) * scale_y - 0.5);
            int sy = cv_floor_f(fy); fy -= sy;
            tables[o2 + dy] = (int16_t)std::max(-32768, std::min(32767, sy));
            tables[o3 + 2 * dy] = sat_short((1.f - fy) * 2048);
            tables[o3 + 2 * dy + 1] = sat_short(fy * 2048);
        }
        V.xmax = xmax;
        V.xofs = at_offset<int16_t>(2 * o0); V.ialpha = at_offset<int16_t>(2 * o0);
        V.yofs = at_offset<int16_t>(2 * o2); V.ibeta = at_offset<int16_t>(2 * o3);
    }
}

// Host side of the quadtree kernel's geometric-key tables (see k_quadtree): the expressions of the kernel's former in-kernel build, evaluated once
// per plan.  Appends level `V`'s tables to `blob` (16-byte granules) and returns their offsets; false = the level does not use them (more than 8 roots
// or a level wider than the tables).  This file is compiled with -ffp-contract=off and IEEE division, like the device code, so the floats agree.
bool quadtree_build_tables(HsLevel& V, std::vector<uint8_t>& blob, size_t& xoff, size_t& yoff)
{
    V.qt_xtab = V.qt_ytab = nullptr;
    for (int i = 0; i < 8; i++) V.qt_rbound[i] = 0;
    const int nIni = V.n_ini;
    if (nIni < 1 || nIni > 8 || V.qt_w <= 0 || V.qt_h <= 0 || V.qt_w >= 8192 - 16 || V.qt_h >= 4096 - 16) return false;
    const float hX = V.hx;
    const int DH = nIni <= 2 ? 6 : 5;
    auto root_of = [&](int x) { return std::min((int)((float)x / hX), nIni - 1); };
    auto descend = [&](int x, int x0, int x1) {
        int idx = 0;
        for (int d = 0; d < DH; d++) {
            const int mx = x0 + ((x1 - x0 + 1) >> 1);
            if (x < mx) { x1 = mx; idx = 2 * idx; } else { x0 = mx; idx = 2 * idx + 1; }
        }
        return idx;
    };
    for (int r = 1; r < nIni; r++) {                                 // smallest x that lands in root r: around r * hX
        int bnd = (int)(hX * (float)r);
        while (bnd > 0 && root_of(bnd - 1) >= r) bnd--;
        while (root_of(bnd) < r) bnd++;
        V.qt_rbound[r] = bnd;
    }
    auto grow = [&](size_t n) { const size_t o = (blob.size() + 15) & ~(size_t)15; blob.resize(o + ((n + 15) & ~(size_t)15), 0); return o; };
    xoff = grow((size_t)V.qt_w + 1);
    for (int x = 0; x <= V.qt_w; x++) {
        const int r = root_of(x);
        blob[xoff + x] = (uint8_t)descend(x, (int16_t)(int)(hX * (float)r), (int16_t)(int)(hX * (float)(r + 1)));
    }
    yoff = grow((size_t)V.qt_h + 1);
    for (int y = 0; y <= V.qt_h; y++) blob[yoff + y] = (uint8_t)descend(y, 0, (int16_t)V.qt_h);
    return true;
}

// Geometric-key tables of the quadtree kernel, and the FAST kernel's side of the same keys (HsFastQt): u16 tables
// xkey[x] = root(x) << 2 DH | spread(xtab[x]),  ykey[y] = spread(ytab[y]) << 1,  padded by 512 entries, and every level's place in the per-image
// histogram / best-candidate arrays
void plan_quadtree_keys(const HsKnobs& k, HsPlan& P)
{
    const int L = (int)P.lv.size();
    std::vector<uint8_t>& qblob = P.qt_tabs;
    std::vector<size_t> xo(L, 0), yo2(L, 0); std::vector<char> has(L, 0);
    for (int l = 0; l < L; l++) {
        has[l] = quadtree_build_tables(P.lv[l], qblob, xo[l], yo2[l]) ? 1 : 0;
        if (has[l]) { P.lv[l].qt_xtab = at_offset<uint8_t>(xo[l]); P.lv[l].qt_ytab = at_offset<uint8_t>(yo2[l]); }
    }
    auto spread = [](uint32_t v) { v = (v | (v << 4)) & 0x0F0Fu; v = (v | (v << 2)) & 0x3333u; v = (v | (v << 1)) & 0x5555u; return v; };
    std::vector<uint16_t>& keys = P.qkeys;
    P.fast_qt.assign(L, HsFastQt{});
    uint32_t hoff = 0, boff = 0;
    for (int l = 0; l < L; l++) {
        HsLevel& V = P.lv[l];
        V.qt_hist_off = V.qt_best_off = 0xFFFFFFFFu;
        // (HS_FAST_KEYS_LEVELS: only levels 0 .. n-1.  Measured at one 1080p pair per call, quadtree us for n = 0 / 1 / 2 / 3 / 8: 35.1 / 32.6 /
        // 31.4 / 30.8 / 24.8 — every level's workgroup is about as long as level 0's, the fixed block-wide steps dominate — so it is all or nothing.)
        if (!has[l] || !k.fast_keys || l >= k.fast_keys_levels) continue;
        const int DH = V.n_ini <= 2 ? 6 : 5, ncell = V.n_ini << (2 * DH);
        const size_t kx = keys.size(); keys.resize(kx + (size_t)V.qt_w + 1 + 512, 0);
        for (int x = 0; x <= V.qt_w; x++) {
            int r = 0;
            for (int i = 1; i < V.n_ini; i++) r += x >= V.qt_rbound[i];
            keys[kx + x] = (uint16_t)(((uint32_t)r << (2 * DH)) | spread(qblob[xo[l] + x]));
        }
        const size_t ky = keys.size(); keys.resize(ky + (size_t)V.qt_h + 1 + 512, 0);
        for (int y = 0; y <= V.qt_h; y++) keys[ky + y] = (uint16_t)(spread(qblob[yo2[l] + y]) << 1);
        V.qt_hist_off = hoff; V.qt_best_off = boff;
        hoff += (uint32_t)(ncell / 2); boff += (uint32_t)ncell;
        HsFastQt& Q = P.fast_qt[l];
        Q.xkey = at_offset<uint16_t>(2 * kx); Q.ykey = at_offset<uint16_t>(2 * ky);
        Q.hist_off = V.qt_hist_off; Q.best_off = V.qt_best_off; Q.enabled = 1;
    }
    P.qhist_stride = hoff; P.qbest_stride = boff;
}

struct Fnv {
    uint64_t v = 0xcbf29ce484222325ull;
    // FNV-1a's xor-then-multiply step, over 8-byte words where there are that many and over bytes for the rest: one multiply per word keeps the
    // pass over the plan's tables (a few hundred KB at 1080p) far below the time the allocations take
    void bytes(const void* p, size_t n)
    {
        const uint8_t* b = static_cast<const uint8_t*>(p);
        for (; n >= 8; n -= 8, b += 8) { uint64_t w; memcpy(&w, b, 8); v ^= w; v *= 0x100000001b3ull; }
        for (; n > 0; n--, b++) { v ^= *b; v *= 0x100000001b3ull; }
    }
    template <class T> void val(const T& x) { static_assert(std::is_arithmetic<T>::value, "fields only: a record may have padding"); bytes(&x, sizeof(T)); }
    void off(const void* p) { val((uint64_t)(uintptr_t)p); }            // a pointer field of the plan: its byte offset
    template <class T> void vec(const std::vector<T>& x) { val((uint64_t)x.size()); if (!x.empty()) bytes(x.data(), x.size() * sizeof(T)); }
};

void hash_level(Fnv& H, const HsLevel& V)          // every field in declaration order (the record has padding after `quota`)
{
    H.val(V.w); H.val(V.h); H.val(V.pitch); H.val(V._r0); H.val(V.img_stride); H.off(V.base);
    H.val(V.ncols); H.val(V.nrows); H.val(V.wcell); H.val(V.hcell); H.val(V.cell_begin);
    H.val(V.grp_cells); H.val(V.ngroups); H.val(V.item_begin); H.val(V.inv_wcell); H.val(V.inv_wcell1);
    H.val(V.qt_w); H.val(V.qt_h); H.val(V.n_ini); H.val(V.hx); H.val(V.quota);
    H.off(V.qt_xtab); H.off(V.qt_ytab); for (int i = 0; i < 8; i++) H.val(V.qt_rbound[i]);
    H.val(V.qt_hist_off); H.val(V.qt_best_off); H.val(V.cand_cap); H.val(V.sel_cap); H.val(V.cand_off); H.val(V.sel_off);
    H.val(V.xmax); H.off(V.xofs); H.off(V.ialpha); H.off(V.yofs); H.off(V.ibeta); H.val(V.scale); H.val(V.kp_size);
    H.val(V.fuse_tbx); H.val(V.fuse_ar); H.val(V.fuse_sr); H.val(V.fuse_pitch); H.val(V.chain_n); H.val(V._r1);
}

// the records below are hashed as bytes: no padding (the sizes are the sums of their fields), and every one starts from a zero-initialised
// record (HsFastQt{}, HsPyrFuse{}, HsPyrChain{} by the planners, memset in hs_plan_fast.hip's build_items)
static_assert(sizeof(HsFastQt) == 32 && sizeof(HsPyrFuse) == 152 && sizeof(HsPyrStage) == 64 && sizeof(HsPyrChain) == 56 + 64 * HS_PYR_CHAIN_MAX && sizeof(HsFastItem) == 64,
              "hs_plan_digest hashes these records as bytes: a record that gains padding must be hashed field by field");

} // namespace

bool hs_quadtree_small_level(const HsLevel& V)
{
    if (V.quota + 8 > HS_QT_LEVEL_NODES) return false;
    if (V.qt_w + 1 > HS_QT_LEVEL_XTAB || V.qt_h + 1 > HS_QT_LEVEL_YTAB) return false;
    if ((long long)((V.w + 63) >> 6) * ((V.h + 63) >> 6) > HS_QT_LEVEL_TILES) return false;
    // the count domain's pyramid one depth above the key tables' (6 for <= 2 roots, else 5), at least 4 deep; more than 8 roots have no tables at all
    if (V.n_ini == 0) return true;                      // a level without a FAST cell: no candidates, no tree
    if (V.n_ini < 1 || V.n_ini > 8) return false;
    const int DH = (V.n_ini <= 2 ? 6 : 5) - 1;
    return DH >= 4 && (long long)V.n_ini * (((1ll << (2 * DH + 2)) - 1) / 3) <= HS_QT_LEVEL_HPYR;
}

int hs_quadtree_small_from(const HsLevel* lv, int nlevels)
{
    int k = nlevels;
    while (k > 0 && hs_quadtree_small_level(lv[k - 1])) k--;
    return k;
}

int hs_plan_geometry(const HsPlanInput& in, HsPlan& P, std::string& err)
{
    P = HsPlan{};
    Refusal r = plan_levels(in, P);
    if (r.code == HS_OK) {
        plan_resize_tables(P);
        plan_quadtree_keys(*in.knobs, P);
        hs_plan_pyramid(*in.knobs, P);
        if (const char* why = hs_plan_fast_items(*in.knobs, P)) r = { HS_ERR_INVALID, why };      // last: the items and the narrow levels copy what the steps above left in the levels
    }
    if (r.code != HS_OK) { err = r.text; return r.code; }
    P.digest = hs_plan_digest(P);
    return HS_OK;
}

// Order: the scalars (w, h, total_cells, max_wcell, max_hcell, fast_items, fast_items_n, cand_img_stride, sel_img_stride, max_kp, qhist_stride,
// qbest_stride, pyr_per_img), the wide levels, the narrow levels, the resize tables, the quadtree blob, the key table, the HsFastQt records,
// the pyramid blob, pyr_fuse, pyr_chain, pyr_deep, the wide items, the narrow items.  The column records (pyr_cols and the offsets into it) are NOT
// hashed: they are derived from what is — the x tables and the tile records — by hs_pyramid_col_records, and tests/test_pyramid_columns.py holds every
// one of them to those, so the digest still decides what the kernels get and keeps the values recorded for it.  Arrays are preceded by their length.
uint64_t hs_plan_digest(const HsPlan& P)
{
    Fnv H;
    H.val(P.w); H.val(P.h); H.val(P.total_cells); H.val(P.max_wcell); H.val(P.max_hcell); H.val(P.fast_items); H.val(P.fast_items_n);
    H.val(P.cand_img_stride); H.val(P.sel_img_stride); H.val(P.max_kp); H.val(P.qhist_stride); H.val(P.qbest_stride); H.val((uint64_t)P.pyr_per_img);
    for (const std::vector<HsLevel>* lv : { &P.lv, &P.lv_n }) { H.val((uint64_t)lv->size()); for (const HsLevel& V : *lv) hash_level(H, V); }
    H.vec(P.tables); H.vec(P.qt_tabs); H.vec(P.qkeys); H.vec(P.fast_qt); H.vec(P.pyr_tabs);
    H.vec(P.pyr_fuse); H.vec(P.pyr_chain); H.vec(P.pyr_deep);
    H.vec(P.items); H.vec(P.items_n);
    return H.v;
}
