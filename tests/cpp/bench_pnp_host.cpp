// bench_pnp_host.cpp — for scale in tools/bench_pnp.py: what a C++ caller without the batch does, hs_pnp_iterate (the host-pointer form, staged and
// synchronous) once per candidate, one after another.  Reads the problem tools/bench_pnp.py wrote; prints microseconds per round over all candidates.
//   bench_pnp_host <file> <iters>      file: int32 Q, N, H; hs_pnp_params [Q]; hs_pnp_corr [Q * N]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../include/hyslam_amd.h"

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    if (std::fread(hdr, 4, 3, f) != 3) return 2;
    const int Q = hdr[0], N = hdr[1], H = hdr[2], iters = std::atoi(argv[2]);
    std::vector<hs_pnp_params> par(Q);
    std::vector<hs_pnp_corr> corrs((size_t)Q * N);
    if (std::fread(par.data(), sizeof(hs_pnp_params), Q, f) != (size_t)Q || std::fread(corrs.data(), sizeof(hs_pnp_corr), corrs.size(), f) != corrs.size()) return 2;
    std::fclose(f);
    hs_orb_params op; hs_orb_default_params(&op);
    hs_orb* h = nullptr;
    if (hs_orb_create(&op, 0, &h) != HS_OK) return 3;
    std::vector<uint8_t> best(N), inl(N);
    const int64_t off[2] = { 0, N };
    long refined = 0;
    double us = 0;
    for (int it = -3; it < iters; it++) {                          // three warm-up rounds
        const auto t0 = std::chrono::steady_clock::now();
        for (int q = 0; q < Q; q++) {
            hs_pnp_state st; hs_pnp_state_init(&st);
            hs_pnp_result res;
            if (hs_pnp_iterate(h, 1, &par[q], off, corrs.data() + (size_t)q * N, H, nullptr, 0, &st, best.data(), &res, inl.data()) != HS_OK) return 4;
            refined += res.status == HS_PNP_REFINED;
        }
        if (it >= 0) us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    }
    std::printf("%.2f %ld\n", us / iters, refined);
    hs_orb_destroy(h);
    return 0;
}
