// hs_plan_pyramid.hip — the host plan of the image pyramid (hs_plan_geometry's step hs_plan_pyramid): which launches make the levels — fused pairs,
// chains, the small-batch chains — and every record their kernels read (hs_pyramid.h): tile, row and column records.  Pure host code, no HIP call;
// the kernels and the launch function are in kernels_pyramid.hip.  Pointer fields hold byte offsets into their blob until hs_api.hip relocates them.
#include "hs_plan.h"
#include <cstdlib>
#include <cstring>

static inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// n zeroed words at the end of a blob of records, on a multiple of `align` words; returns the index of the first.  Word 0 of a blob is never a record.
static size_t blob_append(std::vector<uint64_t>& blob, size_t n, size_t align = 1)
{
    if (blob.empty()) blob.push_back(0);
    while (blob.size() % align) blob.push_back(0);
    const size_t o = blob.size(); blob.resize(o + n, 0);
    return o;
}

// The record of destination row y: its two source rows — clamped to the source level's `src_h` rows, as byte offsets into a sums buffer whose first
// row is source row `src_first` — and its vertical weights
static HsPyrRow row_record(const int16_t* yofs, const int16_t* ibeta, int y, int src_h, int src_first)
{
    HsPyrRow r;
    r.off0 = (uint16_t)((clampi(yofs[y], 0, src_h - 1) - src_first) * 512); r.off1 = (uint16_t)((clampi(yofs[y] + 1, 0, src_h - 1) - src_first) * 512);
    r.b0 = (uint16_t)ibeta[2 * y]; r.b1 = (uint16_t)ibeta[2 * y + 1];
    return r;
}

// Host side of pyr_col_request / pyr_col_data: the 64 column records of one tile column in the plane layout (HsPyrCol).  Lane t makes
// the columns x0 + 4 t + i, i = 0..3; a column past the level's last one repeats it (its pixels land in the row padding or are never stored).
//   wbase | wshift   byte offset of the lane's 8-byte window in a staged row (origin = first source column the row holds), split into dword and byte part
//   sel[i]           v_perm selector: bytes q, q + 1 of the window as two 16-bit fields, q = sx[i] - sx[0] (a1 == 0 wherever sx + 1 is past the row)
//   coef[i]          16 a0 | 16 a1 << 16
size_t hs_pyramid_col_records(const int16_t* xt, int w, int x0, int origin, std::vector<uint64_t>& blob)
{
    const size_t o = blob_append(blob, HS_PYR_COL_TILE_BYTES / 8, 2);       // the planes are read as 16-byte vectors
    uint32_t* const out = reinterpret_cast<uint32_t*>(&blob[o]);
    for (int t = 0; t < 64; t++) {
        const int16_t* e[4];
        for (int i = 0; i < 4; i++) e[i] = xt + 4 * (size_t)std::min(x0 + 4 * t + i, w - 1);
        HsPyrCol c;
        const int o0 = e[0][0] - origin;
        c.wbase = o0 & ~3; c.wshift = o0 & 3;
        for (int i = 0; i < 4; i++) {
            const uint32_t q = (uint32_t)(e[i][0] - e[0][0]);
            c.sel[i] = q | 0x0c00u | ((q + 1) << 16) | 0x0c000000u;
            c.coef[i] = ((uint32_t)(uint16_t)e[i][1] << 4) | ((uint32_t)(uint16_t)e[i][2] << 20);
        }
        uint32_t* const p0 = out + 4 * t, * const p1 = out + 256 + 4 * t, * const p2 = out + 512 + 4 * t;
        p0[0] = (uint32_t)c.wbase; p0[1] = (uint32_t)c.wshift; p0[2] = c.sel[0]; p0[3] = c.sel[1];
        p1[0] = c.sel[2]; p1[1] = c.sel[3]; p1[2] = c.coef[0]; p1[3] = c.coef[1];
        p2[0] = c.coef[2]; p2[1] = c.coef[3];
    }
    return o * 8;
}
size_t hs_pyramid_level_cols(const int16_t* xt, int w, std::vector<uint64_t>& blob)
{
    size_t first = 0;
    for (int x0 = 0; x0 < w; x0 += 256) {
        const size_t o = hs_pyramid_col_records(xt, w, x0, xt[4 * (size_t)x0] & ~15, blob);
        if (x0 == 0) first = o;
    }
    return first;
}

// ---- a fused pair: levels A = l and B = l + 1 from S = l - 1 in one launch of k_resize_two_levels, a workgroup per tbx x FZ_ROWS tile of B
struct PyrPair {
    const HsLevel& S; const HsLevel& A; const HsLevel& B;
    const int16_t* xA; const int16_t* xB; const int16_t* yA; const int16_t* yB;
    int tbx;
    int nbx() const { return (B.w + tbx - 1) / tbx; }
    int nby() const { return (B.h + FZ_ROWS - 1) / FZ_ROWS; }
};
// Tile column bx: its level-A region starts at the first source column of the tile (ax0) and is OWNED up to the next tile's start; the source rectangle is
// sized for the worst case of 256 region columns, in 16-byte vectors from a 16-aligned first column
static HsPyrXTile pair_xtile(const PyrPair& p, int bx)
{
    const int bx0 = bx * p.tbx; const bool last_x = bx0 + p.tbx >= p.B.w;
    HsPyrXTile t{};
    t.ax0 = bx == 0 ? 0 : (p.xB[4 * bx0] & ~3);
    t.own_x1 = last_x ? ((p.A.w + 3) & ~3) : (p.xB[4 * (bx0 + p.tbx)] & ~3);
    const int ax_lastcol = std::min(t.ax0 + 255, p.A.w - 1);
    t.col0 = p.xA[4 * t.ax0] & ~15;
    const int col_last = std::min(p.xA[4 * ax_lastcol] + 1, p.S.w - 1);
    t.nvec = ((col_last - t.col0) >> 4) + 1;
    return t;
}
// Tile row by: the same for the rows — the region ends at the last row the tile reads or owns, and the source rows are those the region reads
static HsPyrYTile pair_ytile(const PyrPair& p, int by)
{
    const int by0 = by * FZ_ROWS, by_last = std::min(by0 + FZ_ROWS, p.B.h) - 1; const bool last_y = by0 + FZ_ROWS >= p.B.h;
    HsPyrYTile t{};
    t.ay0 = by == 0 ? 0 : clampi(p.yB[by0], 0, p.A.h - 1);
    t.own_y1 = last_y ? p.A.h : clampi(p.yB[by0 + FZ_ROWS], 0, p.A.h - 1);
    t.ay_last = std::max(clampi(p.yB[by_last] + 1, 0, p.A.h - 1), t.own_y1 - 1);
    t.sy_first = clampi(p.yA[t.ay0], 0, p.S.h - 1);
    t.n_sr = clampi(p.yA[t.ay_last] + 1, 0, p.S.h - 1) - t.sy_first + 1;
    return t;
}

// Can levels (l, l+1) be fused, and with which tile geometry?  Walks every tile's records and checks what the kernel assumes: the level-A region of
// a tile (owned part + halo) fits 256 columns / fuse_ar rows, its source rectangle fits the LDS rectangle, all LDS fits.
static void hs_pyramid_plan_fusion(HsLevel* h_lv, int nlevels, const int16_t* const* xtab, const int16_t* const* yofs, int tbx_max /*>= 64: cap on the level-B tile width*/)
{
    for (int l = 1; l < nlevels; l++) h_lv[l].fuse_tbx = h_lv[l].fuse_ar = h_lv[l].fuse_sr = h_lv[l].fuse_pitch = 0;
    for (int l = 1; l + 1 < nlevels; l += 2) {
        HsLevel& A = h_lv[l]; const HsLevel& B = h_lv[l + 1]; const HsLevel& S = h_lv[l - 1];
        const double scxA = (double)S.w / A.w, scyA = (double)S.h / A.h, scxB = (double)A.w / B.w, scyB = (double)A.h / B.h;
        if (scxA > 2.0 || scxB > 2.0 || scyA > 2.0 || scyB > 2.0 || B.w < 8 || B.h < 1) continue;
        int tbx = std::min(256, ((int)(250.0 / scxB)) & ~3);
        if (tbx_max >= 64) tbx = std::min(tbx, tbx_max & ~3);      // tuning / experiment knob (HS_PYRAMID_TBX_MAX): narrower level-B tiles
        if (tbx < 64) continue;
        const PyrPair p{ S, A, B, xtab[l], xtab[l + 1], yofs[l], yofs[l + 1], tbx };
        int ar = 0, sr = 0, pitch = 0; bool ok = true;
        for (int by = 0; by < p.nby(); by++) {
            const HsPyrYTile t = pair_ytile(p, by);
            ar = std::max(ar, t.ay_last - t.ay0 + 1);
            sr = std::max(sr, t.n_sr);
        }
        for (int bx = 0; bx < p.nbx() && ok; bx++) {
            const HsPyrXTile t = pair_xtile(p, bx);
            const int bx0 = bx * tbx, need_last = std::min(p.xB[4 * (std::min(bx0 + tbx, B.w) - 1)] + 1, A.w - 1);      // last level-A column the tile reads
            if (p.xB[4 * bx0] < t.ax0 || t.own_x1 - t.ax0 > 256 || need_last - t.ax0 > 255 || t.own_x1 < t.ax0) ok = false;
            // window of the last lane: offset of its first column + 11 bytes must stay inside the LDS row
            if (p.xB[4 * std::min(bx0 + tbx - 4, B.w - 1)] - t.ax0 + 12 > FZ_APITCH) ok = false;
            pitch = std::max(pitch, t.nvec * 16 + 16);
            if (p.xA[4 * t.ax0] < t.col0) ok = false;
        }
        if (!ok) continue;
        pitch = (pitch + 15) & ~15;
        if ((size_t)FZ_APITCH * ar > (size_t)pitch * sr || hs_pyr_fuse_lds(pitch, sr, ar) > 60 * 1024) continue;
        A.fuse_tbx = tbx; A.fuse_ar = ar; A.fuse_sr = sr; A.fuse_pitch = pitch;
    }
}

// Host side of the table-driven kernel: for every fused pair the tile records and for both levels of the pair the row and column records; everything
// is appended to `blob` / `cols_blob`, pointers into them are byte offsets.
static void hs_pyramid_build_tables(const HsLevel* h_lv, int nlevels, const int16_t* const* xtab, const int16_t* const* yofs, const int16_t* const* ibeta,
                                    std::vector<uint64_t>& blob, std::vector<HsPyrFuse>& fuse, std::vector<uint64_t>& cols_blob, std::vector<HsPyrFuseCols>& fuse_cols)
{
    fuse.assign(nlevels, HsPyrFuse{}); fuse_cols.assign(nlevels, HsPyrFuseCols{});
    blob_append(blob, 0);                                          // (word 0 is there whether or not a pair is fused: the digest covers the blob)
    for (int l = 1; l + 1 < nlevels; l++) {
        const HsLevel& A = h_lv[l];
        if (A.fuse_tbx <= 0) continue;
        const HsLevel& B = h_lv[l + 1]; const HsLevel& S = h_lv[l - 1];
        const PyrPair p{ S, A, B, xtab[l], xtab[l + 1], yofs[l], yofs[l + 1], A.fuse_tbx };
        const int tbx = p.tbx, nbx = p.nbx(), nby = p.nby();
        HsPyrFuse& F = fuse[l];
        F.sbase = l == 1 ? nullptr : S.base; F.s_img_stride = S.img_stride; F.spitch = S.pitch;
        F.abase = A.base; F.a_img_stride = A.img_stride; F.apitch = A.pitch; F.aw = A.w; F.ah = A.h;
        F.bbase = B.base; F.b_img_stride = B.img_stride; F.bpitch = B.pitch; F.bw = B.w; F.bh = B.h;
        F.xtA = reinterpret_cast<const HsXTab*>(A.xofs); F.xtB = reinterpret_cast<const HsXTab*>(B.xofs);
        F.tbx = tbx; F.sr = A.fuse_sr; F.lds_pitch = A.fuse_pitch; F.valid = 1;
        std::vector<HsPyrXTile> xt(nbx); std::vector<HsPyrYTile> yt(nby);
        for (int bx = 0; bx < nbx; bx++) xt[bx] = pair_xtile(p, bx);
        for (int by = 0; by < nby; by++) yt[by] = pair_ytile(p, by);
        const size_t ox = blob_append(blob, 4 * (size_t)nbx); memcpy(&blob[ox], xt.data(), 32 * (size_t)nbx);
        const size_t oy = blob_append(blob, 4 * (size_t)nby); memcpy(&blob[oy], yt.data(), 32 * (size_t)nby);
        F.xt = reinterpret_cast<const HsPyrXTile*>(ox * 8); F.yt = reinterpret_cast<const HsPyrYTile*>(oy * 8);
        // row records per y tile (offsets relative to the first row the tile's sums buffer holds), padded with copies of the tile's last row: the
        // kernel prefetches one step of <= 8 rows past the end
        const int slotA = A.fuse_ar + 8, slotB = FZ_ROWS + 8;
        const size_t oa = blob_append(blob, (size_t)slotA * nby), ob = blob_append(blob, (size_t)slotB * nby);
        for (int by = 0; by < nby; by++) {
            const HsPyrYTile& t = yt[by];
            for (int k = 0; k < slotA; k++) {
                const HsPyrRow r = row_record(p.yA, ibeta[l], std::min(t.ay0 + k, t.ay_last), S.h, t.sy_first);
                memcpy(&blob[oa + (size_t)by * slotA + k], &r, 8);
            }
            for (int k = 0; k < slotB; k++) {
                const HsPyrRow r = row_record(p.yB, ibeta[l + 1], std::min(by * FZ_ROWS + k, B.h - 1), A.h, t.ay0);
                memcpy(&blob[ob + (size_t)by * slotB + k], &r, 8);
            }
        }
        F.rowA = reinterpret_cast<const HsPyrRow*>(oa * 8); F.rowB = reinterpret_cast<const HsPyrRow*>(ob * 8); F.slotA = slotA;
        // column records per x tile: level A from the tile's first region column against the staged source rows, level B from the tile's first column
        // against the level-A region in LDS
        for (int pass = 0; pass < 2; pass++)
            for (int bx = 0; bx < nbx; bx++) {
                const HsPyrXTile& t = xt[bx];
                const size_t oc = pass == 0 ? hs_pyramid_col_records(p.xA, A.w, t.ax0, t.col0, cols_blob) : hs_pyramid_col_records(p.xB, B.w, bx * tbx, t.ax0, cols_blob);
                if (bx == 0) (pass == 0 ? fuse_cols[l].a : fuse_cols[l].b) = reinterpret_cast<const uint8_t*>(oc);
            }
    }
}

// Host side of k_resize_chain for the levels [first, first + n), 2 <= n <= HS_PYR_CHAIN_MAX: walks the tiles of the LAST level from the largest tile width
// downwards until every stage's region fits 256 columns and the LDS buffers.  Tile and row records are appended to `blob`, the stages' column records to
// `cols_blob` (offsets until relocated); C.valid = 0 when the geometry does not fit `lds_max` bytes of LDS.  Not the pair's geometry: a chain sizes its
// source rectangle from the columns it really reads, a pair from the worst case of 256.
static void hs_pyramid_plan_chain(const HsLevel* h_lv, int first, int n, const int16_t* const* xtab, const int16_t* const* yofs, const int16_t* const* ibeta,
                                  std::vector<uint64_t>& blob, HsPyrChain& C, std::vector<uint64_t>& cols_blob, HsPyrChainCols& CC, size_t lds_max, int tile_rows /*rows of the last level per tile; 0 = the two-level kernel's*/)
{
    C = HsPyrChain{}; CC = HsPyrChainCols{};
    if (tile_rows <= 0) tile_rows = FZ_ROWS;
    if (n < 2 || n > HS_PYR_CHAIN_MAX || first < 1) return;
    for (int i = 0; i < n; i++) {
        const HsLevel& D = h_lv[first + i]; const HsLevel& S = h_lv[first + i - 1];
        if ((double)S.w / D.w > 2.0 || (double)S.h / D.h > 2.0 || D.w < 8 || D.h < 1) return;
    }
    const HsLevel& LAST = h_lv[first + n - 1];
    const int nby = (LAST.h + tile_rows - 1) / tile_rows;
    // ---- rows (independent of the tile width): part starts, owned ends, regions and source spans — the same three steps as for the columns below
    std::vector<std::vector<HsPyrStageY>> ty(n, std::vector<HsPyrStageY>(nby));
    int h_rows = 0, x_rows0 = 0, x_rows = 0;
    for (int by = 0; by < nby; by++) {
        int y0 = by * tile_rows;
        for (int i = n - 1; i >= 0; i--) {
            ty[i][by] = HsPyrStageY{};
            ty[i][by].y0 = y0;
            if (i > 0) y0 = by == 0 ? 0 : clampi(yofs[first + i][y0], 0, h_lv[first + i - 1].h - 1);
        }
    }
    for (int by = 0; by < nby; by++)
        for (int i = n - 1; i >= 0; i--) {
            HsPyrStageY& t = ty[i][by];
            t.own_y1 = by + 1 < nby ? ty[i][by + 1].y0 : h_lv[first + i].h;
            if (t.own_y1 < t.y0) return;
        }
    for (int by = 0; by < nby; by++) {
        int need_last = std::min(by * tile_rows + tile_rows, LAST.h) - 1;          // last row of the stage's level that is really read
        for (int i = n - 1; i >= 0; i--) {
            const HsLevel& S = h_lv[first + i - 1];
            const int16_t* yo = yofs[first + i];
            HsPyrStageY& t = ty[i][by];
            t.y_last = std::max(need_last, t.own_y1 - 1);
            const int src_first = clampi(yo[t.y0], 0, S.h - 1), src_last = clampi(yo[t.y_last] + 1, 0, S.h - 1);
            if (i > 0) {
                if (src_first < ty[i - 1][by].y0) return;
                t.src_y0 = ty[i - 1][by].y0;
                need_last = src_last;
            } else {
                t.src_y0 = src_first; t.n_src = src_last - src_first + 1;
                x_rows0 = std::max(x_rows0, t.n_src);
                h_rows = std::max(h_rows, t.n_src);
            }
        }
        for (int i = n - 1; i >= 1; i--) {                                          // the source of stage i is the whole region of stage i - 1
            ty[i][by].n_src = ty[i - 1][by].y_last - ty[i - 1][by].y0 + 1;
            x_rows = std::max(x_rows, ty[i][by].n_src);
            h_rows = std::max(h_rows, ty[i][by].n_src);
        }
    }
    // ---- columns: the largest tile width whose regions fit
    std::vector<std::vector<HsPyrStageX>> txs; int tbx, nbx = 0, pitch = 0; size_t x_bytes = 0; bool found = false;
    for (tbx = 256; tbx >= 64; tbx -= 4) {
        nbx = (LAST.w + tbx - 1) / tbx;
        txs.assign(n, std::vector<HsPyrStageX>(nbx));
        bool ok = true; pitch = 0;
        // first columns of every level's parts, last level first (a part starts at the first source column of the tile's part of the level below it)
        for (int bx = 0; bx < nbx; bx++) {
            int x0 = bx * tbx;
            for (int i = n - 1; i >= 0; i--) {
                txs[i][bx] = HsPyrStageX{};
                txs[i][bx].x0 = x0;
                if (i > 0) x0 = bx == 0 ? 0 : (xtab[first + i][4 * x0] & ~3);
            }
        }
        for (int bx = 0; bx < nbx; bx++)
            for (int i = n - 1; i >= 0; i--) {
                const HsLevel& D = h_lv[first + i];
                HsPyrStageX& t = txs[i][bx];
                t.own_x1 = bx + 1 < nbx ? txs[i][bx + 1].x0 : ((D.w + 3) & ~3);
                if (t.own_x1 < t.x0) ok = false;
            }
        // regions: last level = the tile; the level below it must hold the columns the region's last column reads
        for (int bx = 0; bx < nbx && ok; bx++) {
            int need_last = std::min(bx * tbx + tbx, LAST.w) - 1;                  // last column of the region of stage i that is really read
            for (int i = n - 1; i >= 0; i--) {
                const HsLevel& D = h_lv[first + i]; const HsLevel& S = h_lv[first + i - 1];
                HsPyrStageX& t = txs[i][bx];
                const int reg_last = std::max(need_last, std::min(t.own_x1, D.w) - 1);
                t.ncols = ((std::max(reg_last + 1, t.own_x1) - t.x0) + 3) & ~3;
                if (t.ncols > 256 || t.ncols <= 0) { ok = false; break; }
                const int16_t* xt = xtab[first + i];
                const int src_need_first = xt[4 * t.x0], src_need_last = std::min(xt[4 * std::min(reg_last, D.w - 1)] + 1, S.w - 1);
                // the window of the last active lane (offset of its first column + 12 bytes) must stay inside the row of the buffer the stage reads
                const int lastlane_sx = xt[4 * std::min(t.x0 + t.ncols - 4, D.w - 1)];
                if (i > 0) {
                    const HsPyrStageX& u = txs[i - 1][bx];
                    if (src_need_first < u.x0) { ok = false; break; }
                    t.src_x0 = u.x0;
                    if (lastlane_sx - u.x0 + 12 > FZ_APITCH) { ok = false; break; }
                    need_last = src_need_last;
                } else {
                    t.src_x0 = src_need_first & ~15;
                    t.nvec = ((src_need_last - t.src_x0) >> 4) + 1;
                    pitch = std::max(pitch, t.nvec * 16 + 16);
                    if (lastlane_sx - t.src_x0 + 12 > t.nvec * 16 + 16) { ok = false; break; }
                }
            }
        }
        if (!ok) continue;
        pitch = (pitch + 15) & ~15;
        x_bytes = std::max((size_t)pitch * x_rows0, (size_t)FZ_APITCH * x_rows);
        if (hs_pyr_chain_lds(x_bytes, h_rows) > lds_max || h_rows > 127 || x_rows > 127) continue;    // (row records address the sums buffer with 16-bit byte offsets: 512 B per row)
        found = true;
        break;
    }
    if (!found) return;
    // ---- commit
    C.sbase = first == 1 ? nullptr : h_lv[first - 1].base; C.s_img_stride = h_lv[first - 1].img_stride; C.spitch = h_lv[first - 1].pitch; C.nstage = n;
    for (int i = 0; i < n; i++) {
        const HsLevel& D = h_lv[first + i];
        HsPyrStage& S = C.st[i];
        S.base = D.base; S.img_stride = D.img_stride; S.pitch = D.pitch; S.w = D.w; S.h = D.h;
        S.xt = reinterpret_cast<const HsXTab*>(D.xofs);
        // row records per y tile: rows y0 .. y_last of the tile's region, offsets relative to the first row the tile's source buffer holds;
        // every slot is padded with copies of its last row (the kernel prefetches one step of <= 8 rows past the end)
        int slot = 0;
        for (int by = 0; by < nby; by++) slot = std::max(slot, ty[i][by].y_last - ty[i][by].y0 + 1);
        slot += 4 * 8;                                                           // (the vertical pass walks 2 NW rows per step and prefetches one step ahead: 4 NW rows past the end at most)
        const size_t orow = blob_append(blob, (size_t)slot * nby);
        for (int by = 0; by < nby; by++) {
            const HsPyrStageY& t = ty[i][by];
            for (int k = 0; k < slot; k++) {
                const HsPyrRow r = row_record(yofs[first + i], ibeta[first + i], std::min(t.y0 + k, t.y_last), h_lv[first + i - 1].h, t.src_y0);
                memcpy(&blob[orow + (size_t)by * slot + k], &r, 8);
            }
        }
        S.rows = reinterpret_cast<const HsPyrRow*>(orow * 8); S.slot = slot;
        const size_t ox = blob_append(blob, 4 * (size_t)nbx); memcpy(&blob[ox], txs[i].data(), 32 * (size_t)nbx);
        const size_t oy = blob_append(blob, 4 * (size_t)nby); memcpy(&blob[oy], ty[i].data(), 32 * (size_t)nby);
        S.tx = reinterpret_cast<const HsPyrStageX*>(ox * 8); S.ty = reinterpret_cast<const HsPyrStageY*>(oy * 8);
        for (int bx = 0; bx < nbx; bx++) {                                       // column records per x tile: the stage's region columns, window offsets relative to the source buffer's first column
            const size_t oc = hs_pyramid_col_records(xtab[first + i], D.w, txs[i][bx].x0, txs[i][bx].src_x0, cols_blob);
            if (bx == 0) CC.st[i] = reinterpret_cast<const uint8_t*>(oc);
        }
    }
    C.tbx = tbx; C.lds_pitch = pitch; C.x_bytes = (int32_t)((x_bytes + 15) & ~(size_t)15); C.h_rows = h_rows; C.grid_x = nbx; C.grid_y = nby; C.valid = 1;
}

// launches of one hs_launch_pyramid call when every eligible pair is fused (the caller-frame alignment fallback adds one)
int hs_pyramid_launch_count(const HsLevel* h_lv, int nlevels)
{
    int n = 0;
    for (int l = 1; l < nlevels; l++) { n++; if (h_lv[l].chain_n > 0 && l + h_lv[l].chain_n <= nlevels) l += h_lv[l].chain_n - 1; else if (h_lv[l].fuse_tbx > 0 && l + 1 < nlevels) l++; }
    return n;
}

// Which launches make the pyramid: the fused level pairs (decided on the host copies of the resize tables), the chains of the standard plan
// and the small-batch plan.  The planners copy the levels' offsets into their records and append their tile tables to P.pyr_tabs.
void hs_plan_pyramid(const HsKnobs& k, HsPlan& P)
{
    const int L = (int)P.lv.size();
    std::vector<HsLevel>& lv = P.lv;
    std::vector<const int16_t*> xt(L, nullptr), yo(L, nullptr), ib(L, nullptr);
    for (int l = 1; l < L; l++) {
        const uint8_t* const t = reinterpret_cast<const uint8_t*>(P.tables.data());
        xt[l] = reinterpret_cast<const int16_t*>(t + (uintptr_t)lv[l].xofs); yo[l] = reinterpret_cast<const int16_t*>(t + (uintptr_t)lv[l].yofs);
        ib[l] = reinterpret_cast<const int16_t*>(t + (uintptr_t)lv[l].ibeta);
    }
    hs_pyramid_plan_fusion(lv.data(), L, xt.data(), yo.data(), k.pyr_tbx_max);
    if (k.no_fuse) for (int l = 0; l < L; l++) lv[l].fuse_tbx = 0;
    std::vector<uint64_t>& blob = P.pyr_tabs;
    std::vector<uint64_t>& cblob = P.pyr_cols;                 // the column records (HsPyrCol): a blob of their own, see hs_plan.h
    hs_pyramid_build_tables(lv.data(), L, xt.data(), yo.data(), ib.data(), blob, P.pyr_fuse, cblob, P.pyr_fuse_cols);
    auto plan_chain = [&](std::vector<HsPyrChain>& C, std::vector<HsPyrChainCols>& CC, int l, int n, size_t lds_max = 60 * 1024, int tile_rows = 0) {
        hs_pyramid_plan_chain(lv.data(), l, n, xt.data(), yo.data(), ib.data(), blob, C[l], cblob, CC[l], lds_max, tile_rows);
        return C[l].valid != 0;
    };
    // chains: the last three levels in one launch when the number of levels to make is odd (8 levels: (1,2) (3,4) (5,6,7))
    P.pyr_chain.assign(L, HsPyrChain{}); P.pyr_chain_cols.assign(L, HsPyrChainCols{});
    for (int l = 0; l < L; l++) lv[l].chain_n = 0;
    if (!k.no_fuse && k.chain_mode != 0) {
        if (k.chain_mode == 2) {
            for (int l = 1; l + 1 < L; l += 2) {
                int n = (l + 3 == L) ? 3 : 2;
                if (!plan_chain(P.pyr_chain, P.pyr_chain_cols, l, n) && n == 3) plan_chain(P.pyr_chain, P.pyr_chain_cols, l, 2);
                if (P.pyr_chain[l].valid) { lv[l].chain_n = P.pyr_chain[l].nstage; if (P.pyr_chain[l].nstage == 3) l++; }
            }
        } else if (k.pyr_plan_set) {      // tuning knob HS_PYRAMID_PLAN: explicit chain lengths from level 1, e.g. "2,3,2" (1 = a single level, 2 = the two-level kernel unless HS_PYRAMID_CHAIN2=1)
            const bool chain2 = k.pyr_chain2 != 0;
            int l = 1;
            for (const char* q = k.pyr_plan.c_str(); *q && l < L; ) {
                const int n = std::min(atoi(q), L - l);
                if (n >= 3 || (n == 2 && (chain2 || !(l & 1))))         // (the two-level kernel is planned for pairs that start on an odd level)
                    if (plan_chain(P.pyr_chain, P.pyr_chain_cols, l, n, HS_PYR_DEEP_LDS)) lv[l].chain_n = n;
                if (n == 1) lv[l].fuse_tbx = 0;
                l += std::max(n, 1);
                while (*q && *q != ',') q++;
                if (*q == ',') q++;
            }
        } else if (L >= 4 && ((L - 1) & 1)) {
            const int l = L - 3;
            if (plan_chain(P.pyr_chain, P.pyr_chain_cols, l, 3)) lv[l].chain_n = 3;
        }
    }
    // a level made on its own (a pair that is not fused, the level after a pair that fell back for the caller's frame alignment): its column records
    P.pyr_level_cols.assign(L, nullptr);
    for (int l = 1; l < L; l++) P.pyr_level_cols[l] = reinterpret_cast<const uint8_t*>(hs_pyramid_level_cols(xt[l], lv[l].w, cblob));
    // the small-batch plan: a launch of few frames lasts as long as one workgroup lives and costs ~5 us whatever it does, so the dependent
    // launches are what counts — greedy: from level 1, the longest chain that fits HS_PYR_DEEP_LDS, then the next (1080p: ONE launch for levels 1-7)
    P.pyr_deep.assign(L, HsPyrChain{}); P.pyr_deep_cols.assign(L, HsPyrChainCols{});
    if (!k.no_fuse && k.deep_max_batch > 0) {
        for (int l = 1; l + 1 < L;) {
            int took = 0;
            for (int n = std::min(HS_PYR_CHAIN_MAX, L - l); n >= 2 && !took; n--)
                if (plan_chain(P.pyr_deep, P.pyr_deep_cols, l, n, HS_PYR_DEEP_LDS, k.deep_rows)) took = n;
            l += took ? took : 1;
        }
    }
}
