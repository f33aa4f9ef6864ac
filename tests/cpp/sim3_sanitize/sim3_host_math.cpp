// sim3_host_math.cpp — TEST: the __host__ __device__ math of hyslam_amd/csrc/kernels_sim3.hip (sim3_sample, sim3_solve, sim3_transforms, sim3_record,
// sim3_inlier, sim3_walk: the same source the two kernels run) as a host program, so that tests/test_sim3_abi.py can hold it to tests/ref_sim3.py bit
// for bit without a device.  For every iteration of the file's problem: the sample, ComputeSim3 on it, the inlier count and the mask; then the walk
// over the counts.  Floats are printed as hexadecimal floats.
//   sim3_host_math <file> [<draws>] [--samples]
//     file: int32 N, n_hypotheses, fix_scale, min_inliers; uint64 seed; float k1[4], k2[4]; hs_sim3_corr [N]
//     draws: a table of uint32 [cap][HS_SIM3_DRAW_STRIDE] that directs the samples of the first cap iterations (none: the generator alone)
//     --samples: the S lines only, no ComputeSim3 and no walk
#include "kernels_sim3.hip"
#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char** argv)
{
    const char* files[2] = { nullptr, nullptr };
    bool samples_only = false;
    for (int a = 1, n = 0; a < argc; a++) {
        if (!std::strcmp(argv[a], "--samples")) samples_only = true;
        else if (n < 2) files[n++] = argv[a];
    }
    if (!files[0]) return 2;
    std::vector<uint32_t> draws;
    if (files[1]) {
        FILE* d = std::fopen(files[1], "rb");
        if (!d) return 2;
        uint32_t row[HS_SIM3_DRAW_STRIDE];
        while (std::fread(row, 4, HS_SIM3_DRAW_STRIDE, d) == HS_SIM3_DRAW_STRIDE) draws.insert(draws.end(), row, row + HS_SIM3_DRAW_STRIDE);
        std::fclose(d);
    }
    const int draw_cap = (int)(draws.size() / HS_SIM3_DRAW_STRIDE);
    FILE* f = std::fopen(files[0], "rb");
    if (!f) return 2;
    int32_t hdr[4]; unsigned long long seed; float k[8];
    if (std::fread(hdr, 4, 4, f) != 4 || std::fread(&seed, 8, 1, f) != 1 || std::fread(k, 4, 8, f) != 8) return 2;
    const int N = hdr[0], nh = hdr[1];
    if (N < 3 || nh < 0) return 2;
    std::vector<hs_sim3_corr> corrs(N);
    if (std::fread(corrs.data(), sizeof(hs_sim3_corr), N, f) != (size_t)N) return 2;
    std::fclose(f);
    HsSim3Problem p{};
    p.n = N; p.seed = seed; p.q = 0; p.fix_scale = hdr[2]; p.min_inliers = hdr[3];
    for (int i = 0; i < 4; i++) { p.k1[i] = k[i]; p.k2[i] = k[4 + i]; }
    std::vector<int> counts;
    for (int it = 0; it < nh; it++) {
        int s[3];
        sim3_sample(p, it, draw_cap ? draws.data() : nullptr, draw_cap, s);
        std::printf("S %d %d %d %d\n", it, s[0], s[1], s[2]);
        if (samples_only) continue;
        float x1[3][3], x2[3][3];
        for (int a = 0; a < 3; a++)
            for (int r = 0; r < 3; r++) { x1[a][r] = corrs[s[a]].X1c[r]; x2[a][r] = corrs[s[a]].X2c[r]; }
        Sim3Pose o; Sim3Xf xf;
        sim3_solve(x1, x2, p.fix_scale, &o);
        sim3_transforms(o, &xf);
        int cnt = 0;
        std::printf("M %d ", it);
        for (int i = 0; i < N; i++) {
            float r[SIM3_REC];
            sim3_record(corrs[i], p.k1, p.k2, r);
            const bool in = sim3_inlier(xf, p.k1, p.k2, r);
            cnt += in ? 1 : 0;
            std::putchar(in ? '1' : '0');
        }
        std::printf("\nH %d %d", it, cnt);
        for (int i = 0; i < 9; i++) std::printf(" %a", (double)o.R[i]);
        for (int i = 0; i < 3; i++) std::printf(" %a", (double)o.t[i]);
        std::printf(" %a", (double)o.s);
        for (int i = 0; i < 12; i++) std::printf(" %a", (double)xf.a[i]);
        for (int i = 0; i < 12; i++) std::printf(" %a", (double)xf.b[i]);
        std::printf("\n");
        counts.push_back(cnt);
    }
    if (samples_only) return 0;
    int best = 0, rec = -1;
    const int found = sim3_walk(counts.data(), (int)counts.size(), 0, p.min_inliers, &best, &rec);
    std::printf("W %d %d %d\n", found, rec, best);
    return 0;
}
