// test_pyramid_columns.cpp — the column records of the pyramid's LDS-staged kernels (HsPyrCol, hs_pyramid_col_records) against the expressions the kernels
// used to evaluate per workgroup, restated here from the x tables.  No GPU: the library's host code on the stand-in runtime of tests/cpp/host_sanitize
// (device memory = host memory), so the records are read where hs_api.hip relocated and uploaded them.  tests/test_pyramid_columns.py builds this with
// ASan + UBSan and runs it.
// For every frame size on the command line and every knob setting below: every tile column and all 64 lanes of
//   both levels of every fused pair (k_resize_two_levels), every stage of every chain of the standard and the small-batch plan (k_resize_chain),
//   every level on its own (k_resize_level_lds),
// lanes past the level's last column and lanes past the tile width included; and for every lane that reads its window, 0 <= wbase and
// wbase + 12 <= the bytes of a staged row.
// usage: test_pyramid_columns W H [W H ...]        prints "PYRAMID COLUMNS OK ..."
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include "../../hyslam_amd/csrc/hs_internal.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)
static const int APITCH = 272;      // restated, not included: the value of hs_pyramid.h's FZ_APITCH, the LDS pitch of a region a later pass reads

struct Tally { long tiles = 0, lanes = 0, past_w = 0, past_tile = 0, fused = 0, stages = 0, deep_stages = 0, levels = 0, odd_pairs = 0; };

// one tile column: lane t makes columns x0 + 4 t + i; `active` lanes read their window from rows of `row_bytes` bytes
static int check_tile(const char* what, int l, int bx, const uint8_t* tile, const HsXTab* xt, int w, int x0, int origin, int active, int row_bytes, Tally& T)
{
    const uint32_t* const p = reinterpret_cast<const uint32_t*>(tile);
    for (int t = 0; t < 64; t++) {
        // ---- what col_fetch / col_data gave: the lane's four x-table entries, clamped to the level's last column
        HsXTab e[4];
        for (int i = 0; i < 4; i++) e[i] = xt[std::min(x0 + 4 * t + i, w - 1)];
        const int o0 = e[0].sx - origin;
        const int wbase = o0 & ~3, wshift = o0 & 3;
        uint32_t sel[4], coef[4];
        for (int i = 0; i < 4; i++) {
            const uint32_t q = (uint32_t)(e[i].sx - e[0].sx);
            sel[i] = q | 0x0c00u | ((q + 1) << 16) | 0x0c000000u;
            coef[i] = ((uint32_t)(uint16_t)e[i].a0 << 4) | ((uint32_t)(uint16_t)e[i].a1 << 20);
        }
        // ---- the record: three planes of 64 x 16 bytes
        const uint32_t* p0 = p + 4 * t, * p1 = p + 256 + 4 * t, * p2 = p + 512 + 4 * t;
        const uint32_t want[12] = { (uint32_t)wbase, (uint32_t)wshift, sel[0], sel[1], sel[2], sel[3], coef[0], coef[1], coef[2], coef[3], 0u, 0u };
        const uint32_t got[12] = { p0[0], p0[1], p0[2], p0[3], p1[0], p1[1], p1[2], p1[3], p2[0], p2[1], p2[2], p2[3] };
        for (int k = 0; k < 12; k++)
            if (got[k] != want[k]) { printf("FAILED %s level %d tile column %d lane %d word %d: record %08x, x tables give %08x\n", what, l, bx, t, k, got[k], want[k]); return 1; }
        if (t < active && (wbase < 0 || wbase + 12 > row_bytes)) { printf("FAILED %s level %d tile column %d lane %d: window at %d of a %d-byte row\n", what, l, bx, t, wbase, row_bytes); return 1; }
        T.lanes++; T.past_w += x0 + 4 * t + 3 > w - 1; T.past_tile += t >= active;
    }
    T.tiles++;
    return 0;
}

static int check_chain(const char* what, const HsPyrChain& C, const HsPyrChainCols& K, int first, Tally& T, long& stages)
{
    for (int i = 0; i < C.nstage; i++) {
        const HsPyrStage& S = C.st[i];
        CHECK(K.st[i] != nullptr && ((uintptr_t)K.st[i] & 15) == 0);
        for (int bx = 0; bx < C.grid_x; bx++) {
            const HsPyrStageX& X = S.tx[bx];
            CHECK(X.ncols > 0 && X.ncols <= 256);
            if (check_tile(what, first + i, bx, K.st[i] + (size_t)bx * HS_PYR_COL_TILE_BYTES, S.xt, S.w, X.x0, X.src_x0, X.ncols / 4, i == 0 ? C.lds_pitch : APITCH, T)) return 1;
        }
        stages++;
    }
    return 0;
}

static int check_handle(int w, int h, Tally& T)
{
    hs_orb_params p; hs_orb_default_params(&p);
    p.nfeatures = 500; p.scale_factor = 1.2f; p.nlevels = 8;
    hs_orb* ex = nullptr;
    CHECK(hs_orb_create(&p, 0, &ex) == HS_OK);
    CHECK(hs_orb_reserve(ex, w, h, 3) == HS_OK);
    HsDebugPyramidPlan P; hs_debug_pyramid_plan(ex, &P);
    CHECK(P.nlevels == 8 && P.lv && P.fuse && P.chain && P.deep && P.cols.fuse && P.cols.chain && P.cols.deep && P.cols.level);
    const int L = P.nlevels;
    for (int l = 1; l < L; l++) {
        const HsLevel& D = P.lv[l]; const HsLevel& S = P.lv[l - 1];
        const HsXTab* const xt = reinterpret_cast<const HsXTab*>(D.xofs);
        // ---- the level on its own: tiles of 256 columns, origin = the tile's first source column rounded down to 16; every lane reads its window
        CHECK(P.cols.level[l] != nullptr && ((uintptr_t)P.cols.level[l] & 15) == 0);
        const double scx = (double)S.w / D.w;
        const int lds_pitch = (((int)(256 * scx) + 2 + 15 + 15) & ~15) + 16;        // hs_launch_pyramid's row of the source rectangle
        for (int bx = 0; bx * 256 < D.w; bx++)
            if (check_tile("single", l, bx, P.cols.level[l] + (size_t)bx * HS_PYR_COL_TILE_BYTES, xt, D.w, 256 * bx, xt[256 * bx].sx & ~15, 64, scx <= 2.0 ? lds_pitch : 1 << 30, T)) return 1;
        T.levels++;
        // ---- the pair (l, l + 1) of the two-level kernel
        const HsPyrFuse& F = P.fuse[l]; const HsPyrFuseCols& K = P.cols.fuse[l];
        if (!F.valid) CHECK(K.a == nullptr && K.b == nullptr);
        if (F.valid) {
            CHECK(l + 1 < L && K.a != nullptr && K.b != nullptr && (((uintptr_t)K.a | (uintptr_t)K.b) & 15) == 0);
            CHECK(F.xtA == xt && F.aw == D.w && F.bw == P.lv[l + 1].w && F.tbx >= 64 && F.tbx <= 256);
            const int nbx = (F.bw + F.tbx - 1) / F.tbx;
            for (int bx = 0; bx < nbx; bx++) {
                const HsPyrXTile& X = F.xt[bx];
                if (check_tile("pair, level A", l, bx, K.a + (size_t)bx * HS_PYR_COL_TILE_BYTES, F.xtA, F.aw, X.ax0, X.col0, 64, F.lds_pitch, T)) return 1;
                if (check_tile("pair, level B", l + 1, bx, K.b + (size_t)bx * HS_PYR_COL_TILE_BYTES, F.xtB, F.bw, bx * F.tbx, X.ax0, F.tbx / 4, APITCH, T)) return 1;
            }
            T.fused++; T.odd_pairs += (F.aw & 3) != 0 && (F.bw & 3) != 0;
        }
        if (P.chain[l].valid && check_chain("chain", P.chain[l], P.cols.chain[l], l, T, T.stages)) return 1;
        if (P.deep[l].valid && check_chain("small-batch chain", P.deep[l], P.cols.deep[l], l, T, T.deep_stages)) return 1;
    }
    hs_orb_destroy(ex);
    return 0;
}

int main(int argc, char** argv)
{
    CHECK(argc >= 3 && (argc & 1));
    static const char* const KNOBS[] = { "HS_PYRAMID_NO_FUSE", "HS_PYRAMID_CHAIN", "HS_PYRAMID_DEEP_MAX" };
    static const char* const SETTINGS[4][3] = { { nullptr, nullptr, nullptr }, { "1", nullptr, nullptr }, { nullptr, "0", "0" }, { nullptr, "2", "0" } };      // the product, level_lds, two_levels, chain_pairs
    Tally T;
    for (int a = 1; a + 1 < argc; a += 2) {
        const int w = atoi(argv[a]), h = atoi(argv[a + 1]);
        for (const auto& s : SETTINGS) {
            for (int k = 0; k < 3; k++) { if (s[k]) setenv(KNOBS[k], s[k], 1); else unsetenv(KNOBS[k]); }
            Tally t;
            if (check_handle(w, h, t)) { printf("at %d x %d, %s=%s %s=%s %s=%s\n", w, h, KNOBS[0], s[0] ? s[0] : "-", KNOBS[1], s[1] ? s[1] : "-", KNOBS[2], s[2] ? s[2] : "-"); return 1; }
            printf("%d x %d [%s %s %s]: %ld fused pairs, %ld chain stages, %ld small-batch stages, %ld tile columns\n", w, h, s[0] ? s[0] : "-", s[1] ? s[1] : "-", s[2] ? s[2] : "-", t.fused, t.stages, t.deep_stages, t.tiles);
            T.tiles += t.tiles; T.lanes += t.lanes; T.past_w += t.past_w; T.past_tile += t.past_tile; T.fused += t.fused; T.stages += t.stages; T.deep_stages += t.deep_stages;
            T.levels += t.levels; T.odd_pairs += t.odd_pairs;
        }
    }
    // every kind of record was met, and so were the lanes that can go wrong
    CHECK(T.fused > 0 && T.stages > 0 && T.deep_stages > 0 && T.levels > 0 && T.past_w > 0 && T.past_tile > 0 && T.odd_pairs > 0);
    printf("PYRAMID COLUMNS OK: %ld records of %ld tile columns (%ld past the last column, %ld past the tile); %ld fused pairs (%ld with both widths off a multiple of 4), %ld + %ld chain stages, %ld single levels\n",
           T.lanes, T.tiles, T.past_w, T.past_tile, T.fused, T.odd_pairs, T.stages, T.deep_stages, T.levels);
    return 0;
}
