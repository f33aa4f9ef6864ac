// pnp_host_math.cpp — TEST: the __host__ __device__ math of hyslam_amd/csrc/kernels_pnp.hip (pnp_sample, pnp_epnp, pnp_inlier: the same source the two
// kernels run, with one "lane" on the host) as a host program, so that tests/test_pnp_abi.py can hold it to LITERAL of tests/ref_pnp.py bit for bit
// without a device.  For every iteration of the file's problem: the sample, EPnP on it, the inlier count; where the count reaches min_inliers, EPnP
// over those inliers and the recount (what Refine() does with that set).  Doubles are printed as hexadecimal floats.
//   pnp_host_math <file> [<draws>] [--samples]
//     file: int32 N, min_set, n_hypotheses, min_inliers; uint64 seed; float th2, fx, fy, cx, cy; hs_pnp_corr [N]
//     draws: a table of uint32 [cap][HS_PNP_MAX_SET] that directs the samples of the first cap iterations (none: the generator alone)
//     --samples: the S lines only, no EPnP
#include "kernels_pnp.hip"
#include <cstdio>
#include <cstring>
#include <vector>

static void put(const char* tag, int it, int cnt, const PnpWs& ws)
{
    std::printf("%s %d %d", tag, it, cnt);
    for (int i = 0; i < 9; i++) std::printf(" %a", ws.R[i]);
    for (int i = 0; i < 3; i++) std::printf(" %a", ws.t[i]);
    std::printf("\n");
}

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
        uint32_t row[HS_PNP_MAX_SET];
        while (std::fread(row, 4, HS_PNP_MAX_SET, d) == HS_PNP_MAX_SET) draws.insert(draws.end(), row, row + HS_PNP_MAX_SET);
        std::fclose(d);
    }
    const int draw_cap = (int)(draws.size() / HS_PNP_MAX_SET);
    FILE* f = std::fopen(files[0], "rb");
    if (!f) return 2;
    int32_t hdr[4]; unsigned long long seed; float c5[5];
    if (std::fread(hdr, 4, 4, f) != 4 || std::fread(&seed, 8, 1, f) != 1 || std::fread(c5, 4, 5, f) != 5) return 2;
    const int N = hdr[0], ms = hdr[1], nh = hdr[2], min_inliers = hdr[3];
    if (N < ms || ms < 4 || ms > HS_PNP_MAX_SET) return 2;
    std::vector<hs_pnp_corr> corrs(N);
    if (std::fread(corrs.data(), sizeof(hs_pnp_corr), N, f) != (size_t)N) return 2;
    std::fclose(f);
    HsPnpProblem p{};
    p.n = N; p.min_set = ms; p.seed = seed; p.q = 0;
    const PnpCam cam{ (double)c5[1], (double)c5[2], (double)c5[3], (double)c5[4] };
    static PnpWs ws;
    auto load = [&](int i, double* d) { const hs_pnp_corr& c = corrs[i]; d[0] = c.Xw[0]; d[1] = c.Xw[1]; d[2] = c.Xw[2]; d[3] = c.u; d[4] = c.v; };
    for (int it = 0; it < nh; it++) {
        int s[HS_PNP_MAX_SET];
        pnp_sample(p, it, draw_cap ? draws.data() : nullptr, draw_cap, s);
        std::printf("S %d", it);
        for (int k = 0; k < ms; k++) { std::printf(" %d", s[k]); load(s[k], ws.pts + 5 * k); }
        std::printf("\n");
        if (samples_only) continue;
        pnp_epnp(&ws, ws.pts, ms, cam);
        std::vector<int> in;
        for (int i = 0; i < N; i++) if (pnp_inlier(ws.R, ws.t, cam, corrs[i], c5[0])) in.push_back(i);
        put("H", it, (int)in.size(), ws);
        if ((int)in.size() < min_inliers) continue;
        std::vector<double> pts(5 * in.size());
        for (size_t k = 0; k < in.size(); k++) load(in[k], &pts[5 * k]);
        pnp_epnp(&ws, pts.data(), (int)in.size(), cam);
        int again = 0;
        for (int i = 0; i < N; i++) again += pnp_inlier(ws.R, ws.t, cam, corrs[i], c5[0]) ? 1 : 0;
        put("R", it, again, ws);
    }
    return 0;
}
