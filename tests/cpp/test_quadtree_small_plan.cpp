// Host-only: which levels the plan gives to the quadtree kernel's level instance (hs_quadtree_small_level / hs_quadtree_small_from, hs_plan.hip).
// Prints `name value` lines; tests/test_quadtree_small_plan.py compiles this file with the plan's sources and compares them.
#include "../../hyslam_amd/csrc/hs_plan.h"
#include <cmath>
#include <cstdio>
#include <vector>

static HsLevel level(int w, int h, int quota)
{
    HsLevel V{};
    V.w = w; V.h = h; V.quota = quota;
    V.qt_w = w - 2 * HS_BORDER; V.qt_h = h - 2 * HS_BORDER;
    V.n_ini = (int)roundf((float)V.qt_w / (float)V.qt_h);
    V.ncols = V.nrows = 1;
    return V;
}

// the constructor tables of hs_orb_create (ORBExtractor.cpp:86-118) and the plan of one frame size
static int plan_k(int nfeatures, float scale_factor, int w, int h, bool qt_large, int* levels_ok)
{
    const int L = 8;
    hs_orb_params p{};
    p.nfeatures = nfeatures; p.scale_factor = scale_factor; p.nlevels = L; p.cell_px = 30; p.ini_th_fast = 20; p.min_th_fast = 4; p.fast_threshold = 20;
    std::vector<float> scale(L), inv(L); std::vector<int> quota(L);
    const double sf = p.scale_factor;
    scale[0] = 1.f;
    for (int i = 1; i < L; i++) scale[i] = (float)(scale[i - 1] * sf);
    for (int i = 0; i < L; i++) inv[i] = 1.0f / scale[i];
    const float factor = (float)(1.0f / sf);
    float nDesired = p.nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)L));
    int sum = 0;
    for (int l = 0; l < L - 1; l++) { quota[l] = (int)nearbyintf(nDesired); sum += quota[l]; nDesired *= factor; }
    quota[L - 1] = p.nfeatures - sum > 0 ? p.nfeatures - sum : 0;
    HsKnobs k{};
    k.chain_mode = -1; k.deep_max_batch = 2; k.deep_rows = 8; k.fast_order = 1; k.fast_keys = 1; k.fast_keys_levels = HS_MAX_LEVELS; k.fast_keys_max_batch = 16;
    k.stereo_fuse = 1; k.split_mode = -1; k.qt_small_from = -1; k.qt_small_threads = 256;
    const HsPlanInput in{ &p, inv.data(), scale.data(), quota.data(), &k, qt_large, w, h };
    HsPlan P; std::string err;
    if (hs_plan_geometry(in, P, err) != HS_OK) { printf("error %s\n", err.c_str()); return -1; }
    *levels_ok = 0;
    for (int l = 0; l < L; l++) *levels_ok |= (hs_quadtree_small_level(P.lv[l]) ? 1 : 0) << l;
    printf("quota0 %d\n", quota[0]);
    // the digest is a function of the records alone: asking for the levels leaves it as it was
    printf("digest_unchanged %d\n", hs_plan_digest(P) == P.digest ? 1 : 0);
    return hs_quadtree_small_from(P.lv.data(), L);
}

int main()
{
    // list capacity: quota + 8 = 512 / 513
    printf("quota504 %d\n", (int)hs_quadtree_small_level(level(800, 600, HS_QT_LEVEL_NODES - 8)));
    printf("quota505 %d\n", (int)hs_quadtree_small_level(level(800, 600, HS_QT_LEVEL_NODES - 7)));
    // table extents: qt_w + 1 = 2048 / 2049 (w = qt_w + 32; 2079 x 500 is 33 x 8 = 264 tiles, so the height is kept at 448: 7 rows, 231 tiles), qt_h + 1 = 1024 / 1025
    printf("xtab2048 %d\n", (int)hs_quadtree_small_level(level(2047 + 32, 448, 100)));
    printf("xtab2049 %d\n", (int)hs_quadtree_small_level(level(2048 + 32, 448, 100)));
    printf("ytab1024 %d\n", (int)hs_quadtree_small_level(level(900, 1023 + 32, 100)));
    printf("ytab1025 %d\n", (int)hs_quadtree_small_level(level(900, 1024 + 32, 100)));
    // tiles: 16 x 16 = 256, 17 x 16 = 272 and, one past the limit exactly, a record of 257 x 1 tiles against 256 x 1
    printf("tiles256 %d\n", (int)hs_quadtree_small_level(level(1024, 1024, 100)));
    printf("tiles272 %d\n", (int)hs_quadtree_small_level(level(1025, 1024, 100)));
    { HsLevel V = level(1024, 1024, 100); V.w = 256 * 64; V.h = 64; printf("tiles256x1 %d\n", (int)hs_quadtree_small_level(V)); V.w += 1; printf("tiles257x1 %d\n", (int)hs_quadtree_small_level(V)); }
    // roots: 1, 2, 3, 8 fit (pyramid depth 5, 5, 4, 4), 9 have no key tables
    for (int n : { 1, 2, 3, 8, 9 }) { HsLevel V = level(800, 600, 100); V.n_ini = n; printf("nini%d %d\n", n, (int)hs_quadtree_small_level(V)); }
    { HsLevel V = level(800, 600, 100); V.n_ini = 0; V.ncols = V.nrows = 0; printf("nini0 %d\n", (int)hs_quadtree_small_level(V)); }
    int ok = 0;
    printf("k_1080p_2000 %d\n", plan_k(2000, 1.2f, 1920, 1080, false, &ok)); printf("ok_1080p_2000 %d\n", ok);
    printf("k_1080p_9000 %d\n", plan_k(9000, 1.4f, 1920, 1080, true, &ok)); printf("ok_1080p_9000 %d\n", ok);
    printf("k_imaging_9000 %d\n", plan_k(9000, 1.4f, 4000, 3000, true, &ok)); printf("ok_imaging_9000 %d\n", ok);
    printf("k_416_900 %d\n", plan_k(900, 1.2f, 416, 320, false, &ok)); printf("ok_416_900 %d\n", ok);
    return 0;
}
