// test_work_layout_initial.cpp — HsInitialWork of hyslam_amd/csrc/hs_work.h, the work area of hs_track_initial_work_bytes, checked without the library
// and without a GPU (tests/test_track_initial_abi.py builds this with ASan + UBSan and runs it).  For every (n, L) of the grid of
// tests/test_work_bytes.py the struct is carved over a malloc of exactly bytes() at a 16-byte aligned address, every sub-array is written end to end
// with a byte of its own (a write past the block is the sanitizer's to report), and then read back: a sub-array that overlaps another one lost its
// byte.  The spans are also compared as intervals: pairwise disjoint, inside the block, aligned to their element, and the nested areas are the ones
// the inner structs carve from their own base.
#include "../../hyslam_amd/csrc/hs_work.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {
int g_checks = 0, g_failed = 0;
void check(bool ok, const char* what, int n, int L, long detail)
{
    g_checks++;
    if (!ok && g_failed++ < 20) std::printf("FAILED %s (n = %d, L = %d, detail %ld)\n", what, n, L, detail);
}
size_t dim(int v) { return v < 0 ? 0 : (size_t)v; }
uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }
struct Span { void* p; size_t bytes, align; };

std::vector<Span> spans(const HsInitialWork& w, int n, int L)
{
    const size_t N = dim(n) * 4, Lb = dim(L) * 4;
    const HsLocalMapWork& lm = w.track.local_map;
    return { { w.track.assoc.minw, N, 4 }, { w.track.assoc.maxw, N, 4 }, { w.track.assoc.erased, N, 4 }, { w.track.assoc.jk, Lb, 4 },
             { lm.q_off, 16, 8 }, { lm.n_ordered, 4, 4 }, { lm.points.flag, dim(L), 1 }, { lm.points.block_cnt, (size_t)lm.points.n_blocks * 4, 4 },
             { w.vassoc.view_op, N, 4 }, { w.vassoc.lm_view, Lb, 4 }, { w.vassoc.idx_old, Lb, 4 }, { w.op_view_run, N, 4 }, { w.op_lm_run, N, 4 } };
}

void check_n_L(int n, int L)
{
    const size_t total = HsInitialWork::bytes(n, L);
    check(total >= HsTrackWork::bytes(n, L) + HsVassocWork::bytes(n, L) + 8 * dim(n) + 256, "bytes: the parts and 256 spare", n, L, (long)total);
    unsigned char* block = static_cast<unsigned char*>(std::malloc(total));            // exactly bytes(): one byte more is the sanitizer's
    if (!block) { check(false, "malloc", n, L, (long)total); return; }
    check(addr(block) % 16 == 0, "malloc alignment", n, L, 0);
    std::memset(block, 0xEE, total);
    HsWorkCursor c(block);
    const HsInitialWork w(c, n, L);
    check(c.offset() == total, "the walk ends at bytes()", n, L, (long)c.offset());
    check(w.base == block && w.track.base == block, "the tracking area heads the block", n, L, 0);
    const std::vector<Span> v = spans(w, n, L);
    for (size_t i = 0; i < v.size(); i++) {
        check(addr(v[i].p) >= addr(block) && addr(v[i].p) + v[i].bytes <= addr(block) + total, "inside the block", n, L, (long)i);
        check(addr(v[i].p) % v[i].align == 0, "aligned to its element", n, L, (long)i);
        for (size_t j = 0; j < i; j++)
            check(addr(v[i].p) + v[i].bytes <= addr(v[j].p) || addr(v[j].p) + v[j].bytes <= addr(v[i].p), "disjoint", n, L, (long)(i * 16 + j));
    }
    for (size_t i = 0; i < v.size(); i++) std::memset(v[i].p, (int)(i + 1), v[i].bytes);                    // every sub-array end to end
    for (size_t i = 0; i < v.size(); i++)
        for (size_t k = 0; k < v[i].bytes; k++)
            if (static_cast<unsigned char*>(v[i].p)[k] != i + 1) { check(false, "a sub-array lost its bytes to another", n, L, (long)i); break; }
    size_t spare = 0;                                                                                       // the last 256 bytes belong to nobody
    for (size_t k = total - 256; k < total; k++) spare += block[k] == 0xEE;
    check(spare == 256, "256 spare bytes at the end", n, L, (long)spare);
    // the nested areas are what the stages carve from the same base
    HsWorkCursor ct(block), cv(w.vassoc.base);
    const HsTrackWork t(ct, n, L);
    const HsVassocWork va(cv, n, L);
    check(t.assoc.minw == w.track.assoc.minw && t.assoc.jk == w.track.assoc.jk && t.local_map.base == w.track.local_map.base &&
          t.local_map.points.block_cnt == w.track.local_map.points.block_cnt, "the tracking area alone", n, L, 0);
    check(va.view_op == w.vassoc.view_op && va.lm_view == w.vassoc.lm_view && va.idx_old == w.vassoc.idx_old, "the replay's area alone", n, L, 0);
    check((addr(w.vassoc.base) - addr(block)) % 256 == 0 && addr(w.vassoc.base) - addr(block) == HsTrackWork::bytes(n, L), "the replay's area follows", n, L, 0);
    std::free(block);
}
}  // namespace

int main()
{
    const int N[] = { -1, 0, 1, 31, 32, 33, 63, 64, 65, 2000, 65535 }, L[] = { -1, 0, 1, 255, 256, 257, 1023, 1024, 1025, 50000 };
    for (int n : N) for (int l : L) check_n_L(n, l);
    { HsWorkCursor c; const HsInitialWork w(c, 2000, 50000); check(!w.base && !w.op_view_run && !w.vassoc.idx_old && c.offset() > 0, "counting mode", 2000, 50000, 0); }
    if (g_failed) { std::printf("INITIAL WORK LAYOUT FAILED: %d of %d checks\n", g_failed, g_checks); return 1; }
    std::printf("INITIAL WORK LAYOUT OK: %d checks\n", g_checks);
    return 0;
}
