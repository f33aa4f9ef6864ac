// monoinit_host_math.cpp — TEST: the __host__ __device__ math of hyslam_amd/csrc/kernels_monoinit.hip (the same source the four kernels run) as a
// single-thread host program, so that tests/test_monoinit_abi.py can hold the kernels' __host__ __device__ FUNCTIONS to tests/ref_monoinit.py bit for bit
// without a device, and tools/bench_monoinit.py can time them.  The driver below restates what the kernels' own drivers do around those functions (the
// float sums of Normalize in key order, the first-max selection, std::sort for the rank): those parts of the kernels are held by the GPU tests alone.
//   monoinit_host_math <in> <out> [--repeat R]
//     in:  hs_monoinit_params; int32 n1, n2, draw_cap, pad; float xy1[n1][2]; float xy2[n2][2]; int32 matches12[n1]; uint32 draws[draw_cap][8]
//     out: int32 N, H; float score[2][H]; float model[2][H][9]; hs_monoinit_result; u8 inliers_h[n1], inliers_f[n1]; float p3d[n1][3]; u8 triangulated[n1]
//   --repeat R: runs the estimate R times and prints the milliseconds of one (the output is that of the last)
#define HS_MONOINIT_MATH_ONLY
#include "kernels_monoinit.hip"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Problem {
    hs_monoinit_params par;
    int n1, n2, draw_cap;
    std::vector<float> xy1, xy2;
    std::vector<int32_t> matches;
    std::vector<uint32_t> draws;
};
struct Output {
    int N = 0, H = 0;
    std::vector<float> score, model, p3d;
    hs_monoinit_result res{};
    std::vector<uint8_t> inl_h, inl_f, tri;
};

static void estimate(const Problem& P, Output& O)
{
    const hs_monoinit_params& par = P.par;
    const int n1 = P.n1, n2 = P.n2, H = par.max_iterations;
    const float k[4] = { par.fx, par.fy, par.cx, par.cy };
    O.H = H;
    O.score.assign((size_t)2 * H, 0.f); O.model.assign((size_t)2 * H * 9, 0.f); O.p3d.assign((size_t)n1 * 3, 0.f);
    O.inl_h.assign(n1, 0); O.inl_f.assign(n1, 0); O.tri.assign(n1, 0);
    std::vector<int> m1, m2;
    for (int i = 0; i < n1; i++)
        if ((unsigned)P.matches[i] < (unsigned)n2) { m1.push_back(i); m2.push_back(P.matches[i]); }
    const int n = (int)m1.size();
    O.N = n;
    hs_monoinit_result r{};
    r.n_matches = n;
    if (n < 8) { r.status = HS_MONOINIT_TOO_FEW; O.res = r; return; }
    r.best_solution = -1; r.best_it_h = -1; r.best_it_f = -1; r.cos_parallax = 1.f; r.status = HS_MONOINIT_FAILED;
    // k_mono_prepare
    float mean[4], dev[4], prep[HS_MONO_PREP_WORDS];
    for (int c = 0; c < 4; c++) {
        const std::vector<float>& xy = c < 2 ? P.xy1 : P.xy2;
        const int nn = c < 2 ? n1 : n2;
        float acc = 0.f;
        for (int j = 0; j < nn; j++) acc += xy[2 * j + (c & 1)];
        mean[c] = acc / nn;
        acc = 0.f;
        for (int j = 0; j < nn; j++) acc += fabsf(xy[2 * j + (c & 1)] - mean[c]);
        dev[c] = acc / nn;
    }
    mono_prep(mean, dev, prep);
    // k_mono_hypotheses
    static MonoWs ws;
    const float inv_s2 = mono_inv_sigma2(par.sigma);
    const MonoSampler sp{ n, 0, par.seed };
    for (int it = 0; it < H; it++) {
        int smp[8];
        const int set = 8;
        hs_ransac_sample<8, false>(sp, set, P.draw_cap ? P.draws.data() : nullptr, P.draw_cap, HS_MONOINIT_DRAW_STRIDE, it, smp);
        float a[8][2], b[8][2];
        for (int j = 0; j < 8; j++) {
            mono_normalized(prep, 0, P.xy1[2 * m1[smp[j]]], P.xy1[2 * m1[smp[j]] + 1], a[j]);
            mono_normalized(prep, 1, P.xy2[2 * m2[smp[j]]], P.xy2[2 * m2[smp[j]] + 1], b[j]);
        }
        for (int model = 0; model < 2; model++) {
            float M[9], Mi[9], score = 0.f;
            mono_hypothesis<true>(model, prep, a, b, &ws, M, Mi);
            for (int i = 0; i < n; i++) {
                float chi[2];
                mono_chi(model, M, Mi, P.xy1[2 * m1[i]], P.xy1[2 * m1[i] + 1], P.xy2[2 * m2[i]], P.xy2[2 * m2[i] + 1], inv_s2, chi);
                (void)mono_score_add(model, chi, &score);
            }
            O.score[(size_t)model * H + it] = score;
            for (int e = 0; e < 9; e++) O.model[((size_t)model * H + it) * 9 + e] = M[e];
        }
    }
    // k_mono_select
    for (int model = 0; model < 2; model++) {
        float bs = 0.f; int bi = -1;
        for (int it = 0; it < H; it++) if (O.score[(size_t)model * H + it] > bs) { bs = O.score[(size_t)model * H + it]; bi = it; }
        float M[9] = {}, Mi[9] = {};
        if (bi >= 0) {
            for (int e = 0; e < 9; e++) M[e] = O.model[((size_t)model * H + bi) * 9 + e];
            if (model == 0) mono_inv33(M, Mi);
            for (int i = 0; i < n; i++) {
                float chi[2], unused = 0.f;
                mono_chi(model, M, Mi, P.xy1[2 * m1[i]], P.xy1[2 * m1[i] + 1], P.xy2[2 * m2[i]], P.xy2[2 * m2[i] + 1], inv_s2, chi);
                (model == 0 ? O.inl_h : O.inl_f)[i] = mono_score_add(model, chi, &unused) ? 1 : 0;
            }
        }
        for (int e = 0; e < 9; e++) (model == 0 ? r.H21 : r.F21)[e] = M[e];
        if (model == 0) { r.score_h = bs; r.best_it_h = bi; } else { r.score_f = bs; r.best_it_f = bi; }
    }
    r.rh = r.score_h / (r.score_h + r.score_f);
    r.model = (double)r.rh > 0.40 ? HS_MONOINIT_MODEL_H : HS_MONOINIT_MODEL_F;
    if ((r.model == HS_MONOINIT_MODEL_F && r.best_it_f < 0) || (r.model == HS_MONOINIT_MODEL_H && r.best_it_h < 0)) r.model = HS_MONOINIT_MODEL_NONE;
    O.res = r;
    if (r.model == HS_MONOINIT_MODEL_NONE) return;
    // k_mono_reconstruct
    const std::vector<uint8_t>& mask = r.model == HS_MONOINIT_MODEL_H ? O.inl_h : O.inl_f;
    const int nm = r.model == HS_MONOINIT_MODEL_H ? 8 : 4;
    float R[8][9], t[8][3];
    if (r.model == HS_MONOINIT_MODEL_H) { if (!mono_motions_h(r.H21, k, R, t)) return; }
    else mono_motions_f(r.F21, k, R, t);
    int N_in = 0;
    for (int i = 0; i < n; i++) N_in += mask[i] ? 1 : 0;
    const float th2 = mono_th2(par.sigma);
    const float cos_min = (float)cos((double)par.min_parallax_deg * 3.14159265358979323846 / 180.0);
    int n_good[8] = {}; float cosk[8];
    for (int m = 0; m < 8; m++) cosk[m] = 1.f;
    MonoMotion mm;
    std::vector<float> cs;
    for (int m = 0; m < nm; m++) {
        mono_motion_setup(R[m], t[m], k, &mm);
        cs.clear();
        for (int i = 0; i < n; i++) {
            if (!mask[i]) continue;
            float X[3], cp = 0.f;
            const int code = mono_check_point(mm, k, P.xy1[2 * m1[i]], P.xy1[2 * m1[i] + 1], P.xy2[2 * m2[i]], P.xy2[2 * m2[i] + 1], th2, X, &cp);
            if (code > 0) { cs.push_back(cp); n_good[m] += code == 2 ? 1 : 0; }
        }
        if (n_good[m] > 0) {
            std::sort(cs.begin(), cs.end());
            cosk[m] = cs[std::min(par.min_triangulated, (int)cs.size() - 1)];
        }
    }
    int dec = -1;
    const int win = r.model == HS_MONOINIT_MODEL_H ? mono_decide_h(n_good, cosk, N_in, par.min_triangulated, par.min_frac_triangulated, cos_min, &dec)
                                                   : mono_decide_f(n_good, cosk, N_in, par.min_triangulated, par.min_frac_triangulated, cos_min, &dec);
    for (int m = 0; m < 8; m++) r.n_good[m] = n_good[m];
    r.best_solution = dec;
    r.cos_parallax = dec >= 0 ? cosk[dec] : 1.f;
    if (win >= 0) {
        mono_motion_setup(R[win], t[win], k, &mm);
        for (int i = 0; i < n; i++) {
            if (!mask[i]) continue;
            float X[3], cp = 0.f;
            const int code = mono_check_point(mm, k, P.xy1[2 * m1[i]], P.xy1[2 * m1[i] + 1], P.xy2[2 * m2[i]], P.xy2[2 * m2[i] + 1], th2, X, &cp);
            if (code > 0) {
                for (int e = 0; e < 3; e++) O.p3d[3 * (size_t)m1[i] + e] = X[e];
                if (code == 2) O.tri[m1[i]] = 1;
            }
        }
        bool finite = true;
        for (int e = 0; e < 9; e++) { r.R21[e] = R[win][e]; finite = finite && mono_finite(R[win][e]); }
        for (int e = 0; e < 3; e++) { r.t21[e] = t[win][e]; finite = finite && mono_finite(t[win][e]); }
        r.n_triangulated = n_good[win];
        r.status = !finite ? HS_MONOINIT_NONFINITE : r.model == HS_MONOINIT_MODEL_H ? HS_MONOINIT_OK_H : HS_MONOINIT_OK_F;
    }
    O.res = r;
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    int repeat = 1;
    for (int a = 3; a + 1 < argc; a++) if (!std::strcmp(argv[a], "--repeat")) repeat = std::atoi(argv[a + 1]);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    Problem P;
    int32_t hdr[4];
    if (std::fread(&P.par, sizeof P.par, 1, f) != 1 || std::fread(hdr, 4, 4, f) != 4) return 2;
    P.n1 = hdr[0]; P.n2 = hdr[1]; P.draw_cap = hdr[2];
    if (P.n1 < 0 || P.n2 < 0 || P.draw_cap < 0 || P.par.max_iterations < 1 || P.par.max_iterations > HS_MONOINIT_MAX_ITERATIONS || P.par.min_triangulated < 0) return 2;
    P.xy1.resize((size_t)2 * P.n1); P.xy2.resize((size_t)2 * P.n2); P.matches.resize(P.n1); P.draws.resize((size_t)P.draw_cap * HS_MONOINIT_DRAW_STRIDE);
    if (std::fread(P.xy1.data(), 8, P.n1, f) != (size_t)P.n1 || std::fread(P.xy2.data(), 8, P.n2, f) != (size_t)P.n2 ||
        std::fread(P.matches.data(), 4, P.n1, f) != (size_t)P.n1 || std::fread(P.draws.data(), 32, P.draw_cap, f) != (size_t)P.draw_cap)
        return 2;
    std::fclose(f);
    Output O;
    const auto t0 = std::chrono::steady_clock::now();
    for (int rep = 0; rep < repeat; rep++) estimate(P, O);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / (repeat > 0 ? repeat : 1);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const int32_t head[2] = { O.N, O.H };
    std::fwrite(head, 4, 2, o);
    std::fwrite(O.score.data(), 4, O.score.size(), o);
    std::fwrite(O.model.data(), 4, O.model.size(), o);
    std::fwrite(&O.res, sizeof O.res, 1, o);
    std::fwrite(O.inl_h.data(), 1, O.inl_h.size(), o);
    std::fwrite(O.inl_f.data(), 1, O.inl_f.size(), o);
    std::fwrite(O.p3d.data(), 4, O.p3d.size(), o);
    std::fwrite(O.tri.data(), 1, O.tri.size(), o);
    std::fclose(o);
    std::printf("MONOINIT HOST MATH OK N=%d H=%d status=%d ms=%.4f\n", O.N, O.H, O.res.status, ms);
    return 0;
}
