// test_work_layout.cpp — the layouts of hyslam_amd/csrc/hs_work.h, checked without the library and without a GPU (tests/test_work_bytes.py builds this
// with ASan + UBSan and runs it).  For every layout struct over the grid of tests/golden/work_bytes.json, on a fake base that is 16-byte aligned and no
// more: every sub-array inside [base, base + bytes), pairwise disjoint and aligned to its element type; a nested struct's pointers equal to the
// outer struct's; bytes() equal to the walk's end; the sub-offsets equal to the layout written down here independently.  Then, from stdin, the rows
// "function arguments... bytes" recorded from the reference build: each struct's bytes() reproduces the public size that is made of it.
#include "../../hyslam_amd/csrc/hs_work.h"
#include <cstdio>
#include <cstring>
#include <vector>

namespace {
int g_checks = 0, g_failed = 0;
void check(bool ok, const char* what, long a, long b, long c)
{
    g_checks++;
    if (!ok && g_failed++ < 20) std::printf("FAILED %s (n / L = %ld, L / kf_cap = %ld, detail %ld)\n", what, a, b, c);
}
size_t up(size_t v) { return (v + 255) / 256 * 256; }
size_t dim(int v) { return v < 0 ? 0 : (size_t)v; }
uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

const uintptr_t BASE = 0x7f0000001230;                // 16-byte aligned, not 32: include/hyslam_amd.h promises no more for d_work
struct Span { const void* p; size_t bytes, align; };
void check_spans(const char* what, const std::vector<Span>& v, size_t total, int a, int b)
{
    for (size_t i = 0; i < v.size(); i++) {
        check(addr(v[i].p) >= BASE && addr(v[i].p) + v[i].bytes <= BASE + total, what, a, b, 100 + (long)i);
        check(addr(v[i].p) % v[i].align == 0, what, a, b, 200 + (long)i);
        for (size_t j = 0; j < i; j++)
            check(addr(v[i].p) + v[i].bytes <= addr(v[j].p) || addr(v[j].p) + v[j].bytes <= addr(v[i].p), what, a, b, 300 + (long)(i * 16 + j));
    }
}
size_t off(const void* p) { return addr(p) - BASE; }

std::vector<Span> spans(const HsAssocWork& w, int n, int L) { return { { w.minw, dim(n) * 4, 4 }, { w.maxw, dim(n) * 4, 4 }, { w.erased, dim(n) * 4, 4 }, { w.jk, dim(L) * 4, 4 } }; }
std::vector<Span> spans(const HsVassocWork& w, int n, int L) { return { { w.view_op, dim(n) * 4, 4 }, { w.lm_view, dim(L) * 4, 4 }, { w.idx_old, dim(L) * 4, 4 } }; }
std::vector<Span> spans(const HsLocalPointsWork& w, int L) { return { { w.flag, dim(L), 1 }, { w.block_cnt, (size_t)w.n_blocks * 4, 4 } }; }
std::vector<Span> spans(const HsLocalMapWork& w, int L)
{
    std::vector<Span> v = { { w.q_off, 16, 8 }, { w.n_ordered, 4, 4 } };
    for (const Span& s : spans(w.points, L)) v.push_back(s);
    return v;
}
bool same(const HsAssocWork& a, const HsAssocWork& b) { return a.base == b.base && a.minw == b.minw && a.maxw == b.maxw && a.erased == b.erased && a.jk == b.jk; }
bool same(const HsLocalPointsWork& a, const HsLocalPointsWork& b) { return a.base == b.base && a.flag == b.flag && a.block_cnt == b.block_cnt && a.n_blocks == b.n_blocks; }
bool same(const HsLocalMapWork& a, const HsLocalMapWork& b) { return a.base == b.base && a.q_off == b.q_off && a.n_ordered == b.n_ordered && same(a.points, b.points); }

size_t assoc_bytes(int n, int L) { return (3 * dim(n) + dim(L)) * 4 + 256; }
size_t lp_bytes(int L) { return up(dim(L)) + up((dim(L) + HS_LOCAL_POINTS_BLOCK - 1) / HS_LOCAL_POINTS_BLOCK * 4) + 256; }

void check_n_L(int n, int L)
{
    void* base = reinterpret_cast<void*>(BASE);
    {   // replay in landmark order
        HsWorkCursor c(base);
        const HsAssocWork w(c, n, L);
        check(c.offset() == HsAssocWork::bytes(n, L) && c.offset() == assoc_bytes(n, L), "assoc bytes", n, L, (long)c.offset());
        check(w.base == base && off(w.minw) == 0 && off(w.maxw) == 4 * dim(n) && off(w.erased) == 8 * dim(n) && off(w.jk) == 12 * dim(n), "assoc offsets", n, L, 0);
        check_spans("assoc", spans(w, n, L), c.offset(), n, L);
    }
    {   // replay in view order
        HsWorkCursor c(base);
        const HsVassocWork w(c, n, L);
        check(c.offset() == HsVassocWork::bytes(n, L) && c.offset() == up((dim(n) + 2 * dim(L)) * 4 + 256), "vassoc bytes", n, L, (long)c.offset());
        check(w.base == base && off(w.view_op) == 0 && off(w.lm_view) == 4 * dim(n) && off(w.idx_old) == 4 * (dim(n) + dim(L)), "vassoc offsets", n, L, 0);
        check_spans("vassoc", spans(w, n, L), c.offset(), n, L);
    }
    {   // track: the replay, then the local map
        HsWorkCursor c(base);
        const HsTrackWork w(c, n, L);
        const size_t lm_at = up(assoc_bytes(n, L));
        check(c.offset() == HsTrackWork::bytes(n, L) && c.offset() == lm_at + up(256 + lp_bytes(L)) + 256, "track bytes", n, L, (long)c.offset());
        check(w.base == base && w.assoc.base == base && off(w.local_map.base) == lm_at, "track offsets", n, L, (long)off(w.local_map.base));
        std::vector<Span> v = spans(w.assoc, n, L);
        for (const Span& s : spans(w.local_map, L)) v.push_back(s);
        check_spans("track", v, c.offset(), n, L);
        HsWorkCursor ca(base), cl(w.local_map.base);
        check(same(HsAssocWork(ca, n, L), w.assoc), "track: the replay alone", n, L, 0);
        check(same(HsLocalMapWork(cl, L), w.local_map), "track: the local map alone", n, L, 0);
    }
}

void check_L(int L)
{
    void* base = reinterpret_cast<void*>(BASE);
    {   // local points
        HsWorkCursor c(base);
        const HsLocalPointsWork w(c, L);
        check(c.offset() == HsLocalPointsWork::bytes(L) && c.offset() == lp_bytes(L), "local points bytes", L, L, (long)c.offset());
        check(w.base == base && off(w.flag) == 0 && off(w.block_cnt) == up(dim(L)) && (size_t)w.n_blocks == (dim(L) + HS_LOCAL_POINTS_BLOCK - 1) / HS_LOCAL_POINTS_BLOCK,
              "local points offsets", L, L, w.n_blocks);
        check_spans("local points", spans(w, L), c.offset(), L, L);
    }
    {   // local map: a 256-byte head, then local points
        HsWorkCursor c(base);
        const HsLocalMapWork w(c, L);
        check(c.offset() == HsLocalMapWork::bytes(L) && c.offset() == 256 + lp_bytes(L), "local map bytes", L, L, (long)c.offset());
        check(w.base == base && off(w.q_off) == 0 && off(w.n_ordered) == 16 && off(w.points.base) == 256, "local map offsets", L, L, 0);
        check_spans("local map", spans(w, L), c.offset(), L, L);
        HsWorkCursor cp(w.points.base);
        check(same(HsLocalPointsWork(cp, L), w.points), "local map: the local points alone", L, L, 0);
    }
}

void check_keyframe(int n, int kf_cap)
{
    void* base = reinterpret_cast<void*>(BASE);
    HsWorkCursor c(base);
    const HsKeyframeWork w(c, n, kf_cap);
    check(c.offset() == HsKeyframeWork::bytes(n, kf_cap) && c.offset() == 256 + up(8 * dim(n)) + up(4 * dim(kf_cap)) + 256, "key frame bytes", n, kf_cap, (long)c.offset());
    check(w.base == base && off(w.q_off) == 0 && off(w.vote) == 16 && off(w.keys) == 256 && off(w.weights) == 256 + up(8 * dim(n)), "key frame offsets", n, kf_cap, 0);
    check_spans("key frame", { { w.q_off, 16, 8 }, { w.vote, 12, 4 }, { w.keys, dim(n) * 8, 8 }, { w.weights, dim(kf_cap) * 4, 4 } }, c.offset(), n, kf_cap);
    // a smaller counter row (the entry points carve with T->n_kf <= kf_cap) moves no pointer
    HsWorkCursor c0(base);
    const HsKeyframeWork w0(c0, n, 0);
    check(w0.q_off == w.q_off && w0.vote == w.vote && w0.keys == w.keys && w0.weights == w.weights, "key frame: kf_cap moves no pointer", n, kf_cap, 0);
}

// one recorded row: the struct that makes up the public size
bool golden_row(const char* name, const long long* a, size_t* got)
{
    if (!std::strcmp(name, "hs_track_work_bytes")) *got = HsTrackWork::bytes((int)a[0], (int)a[2]);
    else if (!std::strcmp(name, "hs_local_points_work_bytes")) *got = HsLocalPointsWork::bytes((int)a[0]);
    else if (!std::strcmp(name, "hs_local_map_work_bytes")) *got = HsLocalMapWork::bytes((int)a[0]);
    else if (!std::strcmp(name, "hs_keyframe_work_bytes")) *got = HsKeyframeWork::bytes((int)a[0], (int)a[1]);
    else if (!std::strcmp(name, "hs_track_refkf_work_bytes")) *got = HsVassocWork::bytes((int)a[0], (int)a[2]);
    else return false;
    return true;
}
}  // namespace

int main()
{
    const int N[] = { -1, 0, 1, 31, 32, 33, 63, 64, 65, 2000, 65535 }, L[] = { -1, 0, 1, 255, 256, 257, 1023, 1024, 1025, 50000 }, KF[] = { 0, 1, 63, 64, 65, 1000 };
    for (int l : L) check_L(l);
    for (int n : N) for (int l : L) check_n_L(n, l);
    for (int n : N) for (int k : KF) check_keyframe(n, k);
    // counting mode hands out no address
    { HsWorkCursor c; const HsTrackWork w(c, 2000, 50000); check(!w.base && !w.assoc.jk && !w.local_map.points.block_cnt && c.offset() > 0, "counting mode", 2000, 50000, 0); }

    char line[256];
    int rows = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        char name[64]; long long v[5]; size_t got = 0;
        const int k = std::sscanf(line, "%63s %lld %lld %lld %lld %lld", name, &v[0], &v[1], &v[2], &v[3], &v[4]);
        if (k < 3) continue;
        const bool known = golden_row(name, v, &got);
        check(known && got == (size_t)v[k - 2], name, (long)v[0], (long)v[1], (long)got);
        rows++;
    }
    if (g_failed) { std::printf("WORK LAYOUT FAILED: %d of %d checks\n", g_failed, g_checks); return 1; }
    std::printf("WORK LAYOUT OK: %d checks, %d recorded sizes\n", g_checks, rows);
    return 0;
}
