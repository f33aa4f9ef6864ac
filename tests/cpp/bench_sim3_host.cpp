// bench_sim3_host.cpp — for scale in tools/bench_sim3.py: the __host__ __device__ math of hyslam_amd/csrc/kernels_sim3.hip — the source the two kernels
// run — compiled for the host and run on ONE core: per problem and hypothesis the sample, ComputeSim3, the two transforms and the inlier count over all
// N (the records staged once per problem, as the kernel stages them per chunk), then the walk over the counts and the mask of the chosen hypothesis.
// Reads the problem tools/bench_sim3.py wrote; prints microseconds per round over all problems and the number of problems that found a pose.  Built
// host-only with the kernels and the launcher left out (hipcc -x hip --cuda-host-only -DHS_SIM3_MATH_ONLY): no HIP call, no library to link.
//   bench_sim3_host <file> <iters>      file: int32 Q, N, H; hs_sim3_params [Q]; hs_sim3_corr [Q * N]
#define HS_SIM3_MATH_ONLY
#include "kernels_sim3.hip"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    if (std::fread(hdr, 4, 3, f) != 3) return 2;
    const int Q = hdr[0], N = hdr[1], H = hdr[2], iters = std::atoi(argv[2]);
    if (Q < 1 || N < 3 || H < 1 || iters < 1) return 2;
    std::vector<hs_sim3_params> par(Q);
    std::vector<hs_sim3_corr> corrs((size_t)Q * N);
    if (std::fread(par.data(), sizeof(hs_sim3_params), Q, f) != (size_t)Q || std::fread(corrs.data(), sizeof(hs_sim3_corr), corrs.size(), f) != corrs.size()) return 2;
    std::fclose(f);
    std::vector<float> rec((size_t)N * SIM3_REC);
    std::vector<int> counts(H);
    std::vector<Sim3Pose> poses(H);
    std::vector<uint8_t> mask(N);
    long found_total = 0;
    double us = 0;
    for (int it = -3; it < iters; it++) {                          // three warm-up rounds
        const auto t0 = std::chrono::steady_clock::now();
        for (int q = 0; q < Q; q++) {
            const hs_sim3_params& pp = par[q];
            HsSim3Problem p{};
            p.n = N; p.seed = pp.seed; p.q = 0; p.fix_scale = pp.fix_scale; p.min_inliers = pp.min_inliers;
            p.k1[0] = pp.fx1; p.k1[1] = pp.fy1; p.k1[2] = pp.cx1; p.k1[3] = pp.cy1; p.k2[0] = pp.fx2; p.k2[1] = pp.fy2; p.k2[2] = pp.cx2; p.k2[3] = pp.cy2;
            const hs_sim3_corr* pc = corrs.data() + (size_t)q * N;
            for (int i = 0; i < N; i++) sim3_record(pc[i], p.k1, p.k2, &rec[(size_t)i * SIM3_REC]);
            const int passes = hs_ransac_passes_and(0, pp.max_iterations, H, H);
            for (int j = 0; j < passes; j++) {
                int s[3];
                float x1[3][3], x2[3][3];
                sim3_sample(p, j, nullptr, 0, s);
                for (int k = 0; k < 3; k++)
                    for (int r = 0; r < 3; r++) { x1[k][r] = pc[s[k]].X1c[r]; x2[k][r] = pc[s[k]].X2c[r]; }
                Sim3Xf xf;
                sim3_solve(x1, x2, p.fix_scale, &poses[j]);
                sim3_transforms(poses[j], &xf);
                int cnt = 0;
                for (int i = 0; i < N; i++) cnt += sim3_inlier(xf, p.k1, p.k2, &rec[(size_t)i * SIM3_REC]) ? 1 : 0;
                counts[j] = cnt;
            }
            int best = 0, best_at = -1;
            const int found = sim3_walk(counts.data(), passes, 0, p.min_inliers, &best, &best_at);
            if (best_at >= 0) {
                Sim3Xf xf;
                sim3_transforms(poses[best_at], &xf);
                for (int i = 0; i < N; i++) mask[i] = sim3_inlier(xf, p.k1, p.k2, &rec[(size_t)i * SIM3_REC]) ? 1 : 0;
            }
            found_total += found >= 0;
        }
        if (it >= 0) us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    }
    std::printf("%.2f %ld %d\n", us / iters, found_total, (int)mask[0]);
    return 0;
}
