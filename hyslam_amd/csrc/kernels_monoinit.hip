// kernels_monoinit.hip — monocular initialisation (MonoEstimator, src/initializers/MonoEstimator.cpp).
//   k_mono_prepare      one workgroup per problem: the ordered compaction of matches12 into mvMatches12 (block_scan_excl per chunk, a running base),
//                       N, and Normalize of both frames over ALL their key points: the keys are staged in LDS, HS_MONO_KEY_CHUNK at a time, and four
//                       lanes own the four float sums (x and y of each frame), in key order
//   k_mono_hypotheses   grid (iteration, model, problem), one wave each: the 8-point sample of iteration `it` (the same for both models), the 16x9 or
//                       8x9 system in LDS, its null vector by the shared Jacobi, the model, then the check over all N matches: the lanes form the two
//                       chi-squares of HS_MONO_CHI_CHUNK matches in LDS and lane 0 adds the accepted terms in match order, first then second
//   k_mono_select       one workgroup per problem: the first iteration of the largest score above 0 of each model, its mask recomputed from the
//                       stored model — the same instructions on the same inputs as the score —, RH and the model handed to reconstruction
//   k_mono_reconstruct  one workgroup per problem: the 8 or 4 motions, CheckRT for each with one lane per match (a 4x4 Jacobi in registers), the
//                       parallax as an order statistic found by rank counting, the two decisions, and the winner's points written by a second pass
// Every float sum is owned by one lane and runs in the reference's order; counts are integers; there is no float atomic.  -ffp-contract=off; divide
// and sqrt correctly rounded; every loop has a bound that no input extends.  The math is __host__ __device__ with one "lane" on the host, so a host
// build of this file computes the same bits (tests/cpp/monoinit_sanitize/monoinit_host_math.cpp).
//   k_mono_hypotheses_lane  the other layout of stage 2, one lane per hypothesis: the same bits (hs_debug_monoinit_layout)
#include "hs_monoinit.h"
#include "hs_jacobi.h"
#include "hs_match_device.h"         // block_scan_excl: the library's ordered compaction
#include <algorithm>
#include <cmath>

static_assert(sizeof(hs_monoinit_params) == 48 && sizeof(hs_monoinit_result) == 200 && sizeof(hs_keypoint) == 24, "include/hyslam_amd.h states these layouts");
static_assert(HS_MONO_KEY_CHUNK == 1024, "k_mono_prepare stages one key per thread of its 1024");

#define MONO_HD __host__ __device__
#define MONO_INF (__builtin_huge_valf())

namespace {

struct MonoWs { double G[16 * 9], V[81], sig[9]; int perm[9]; };  // a wave's workspace (LDS on the device)
struct MonoMotion { float R[9], t[3], P2[12], O2[3]; };
struct MonoSampler { int n, q; unsigned long long seed; };

MONO_HD inline bool mono_finite(float v) { return v - v == 0.f; }  // v - v is 0 for a finite v and a NaN otherwise

// ---- D19 / D20: 3x3 products, inverse, determinant, norm -------------------------------------------------------------------------------------
MONO_HD inline void mono_mul33(const float* a, const float* b, float* o)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            o[3 * i + j] = (float)(((double)a[3 * i] * (double)b[j] + (double)a[3 * i + 1] * (double)b[3 + j]) + (double)a[3 * i + 2] * (double)b[6 + j]);
}
MONO_HD inline void mono_mul31(const float* a, const float* x, float* o)
{
    for (int i = 0; i < 3; i++) o[i] = (float)(((double)a[3 * i] * (double)x[0] + (double)a[3 * i + 1] * (double)x[1]) + (double)a[3 * i + 2] * (double)x[2]);
}
MONO_HD inline double mono_det33(const float* a)
{
    const double m0 = a[0], m1 = a[1], m2 = a[2], m3 = a[3], m4 = a[4], m5 = a[5], m6 = a[6], m7 = a[7], m8 = a[8];
    return (m0 * (m4 * m8 - m5 * m7) + m1 * (m5 * m6 - m3 * m8)) + m2 * (m3 * m7 - m4 * m6);
}
MONO_HD inline void mono_inv33(const float* a, float* o)
{
    const double m0 = a[0], m1 = a[1], m2 = a[2], m3 = a[3], m4 = a[4], m5 = a[5], m6 = a[6], m7 = a[7], m8 = a[8];
    const double c0 = m4 * m8 - m5 * m7, c1 = m5 * m6 - m3 * m8, c2 = m3 * m7 - m4 * m6;
    const double det = (m0 * c0 + m1 * c1) + m2 * c2;
    o[0] = (float)(c0 / det); o[1] = (float)((m2 * m7 - m1 * m8) / det); o[2] = (float)((m1 * m5 - m2 * m4) / det);
    o[3] = (float)(c1 / det); o[4] = (float)((m0 * m8 - m2 * m6) / det); o[5] = (float)((m2 * m3 - m0 * m5) / det);
    o[6] = (float)(c2 / det); o[7] = (float)((m1 * m6 - m0 * m7) / det); o[8] = (float)((m0 * m4 - m1 * m3) / det);
}
// v / cv::norm(v)
MONO_HD inline void mono_unit3(float* v)
{
    const double n = sqrt(((double)v[0] * (double)v[0] + (double)v[1] * (double)v[1]) + (double)v[2] * (double)v[2]);
    for (int i = 0; i < 3; i++) v[i] = (float)((double)v[i] / n);
}
// the full SVD of a float 3x3 as the reference holds it: w descending, u by column, vt by row, all narrowed once
MONO_HD inline void mono_svd33(const float* a, float* u, float* w, float* vt)
{
    HsJacobiSolo<3, 3> s;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) s.G[i][j] = (double)a[3 * i + j];
    hs_jacobi_solo(s);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double v[3], g[3], sig;
        hs_solo_column(s, r, v, g, &sig);
        w[r] = (float)sig;
        for (int k = 0; k < 3; k++) { u[3 * k + r] = (float)(g[k] / sig); vt[3 * r + k] = (float)v[k]; }
    }
}

// ---- Normalize (:761-807) ------------------------------------------------------------------------------------------------------------------------
// prep: T1, T2, T2inv, T2t, then mean x, mean y, sX, sY of frame 1 and of frame 2
MONO_HD inline void mono_prep(const float* mean /*[4]*/, const float* dev /*[4]*/, float* prep)
{
    for (int f = 0; f < 2; f++) {
        const float sX = 1.0f / dev[2 * f], sY = 1.0f / dev[2 * f + 1];
        float* T = prep + 9 * f;
        T[0] = sX; T[1] = 0.f; T[2] = -mean[2 * f] * sX; T[3] = 0.f; T[4] = sY; T[5] = -mean[2 * f + 1] * sY; T[6] = 0.f; T[7] = 0.f; T[8] = 1.f;
        prep[36 + 4 * f] = mean[2 * f]; prep[37 + 4 * f] = mean[2 * f + 1]; prep[38 + 4 * f] = sX; prep[39 + 4 * f] = sY;
    }
    mono_inv33(prep + 9, prep + 18);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) prep[27 + 3 * i + j] = prep[9 + 3 * j + i];
    for (int i = 44; i < HS_MONO_PREP_WORDS; i++) prep[i] = 0.f;
}
MONO_HD inline void mono_normalized(const float* prep, int frame, float x, float y, float* o)
{
    const float* m = prep + 36 + 4 * frame;
    o[0] = (x - m[0]) * m[2]; o[1] = (y - m[1]) * m[3];
}

// ---- ComputeH21 / ComputeF21 (:239-316) and the denormalisation (:172-174, :223-225) ---------------------------------------------------------------
// model 0: H21 = T2inv Hn T1 into M, H12 = H21^-1 into Minv; model 1: F21 = T2t Fn T1 into M.  a, b: the 8 normalised points of frames 1 and 2.
// WAVE: the 64 lanes of a workgroup share ws (LDS) and all call it; !WAVE: the calling lane alone on a ws of its own.
template <bool WAVE> MONO_HD inline void mono_hypothesis(int model, const float* prep, const float (*a)[2], const float (*b)[2], MonoWs* ws, float* M, float* Minv)
{
    const int lane = WAVE ? HS_JACOBI_LANE : 0, rows = model == 0 ? 16 : 8;
    for (int r = lane; r < rows; r += (WAVE ? HS_JACOBI_LANES : 1)) {
        const int i = model == 0 ? r >> 1 : r;
        const float u1 = a[i][0], v1 = a[i][1], u2 = b[i][0], v2 = b[i][1];
        float row[9];
        if (model == 1) { row[0] = u2 * u1; row[1] = u2 * v1; row[2] = u2; row[3] = v2 * u1; row[4] = v2 * v1; row[5] = v2; row[6] = u1; row[7] = v1; row[8] = 1.f; }
        else if ((r & 1) == 0) { row[0] = 0.f; row[1] = 0.f; row[2] = 0.f; row[3] = -u1; row[4] = -v1; row[5] = -1.f; row[6] = v2 * u1; row[7] = v2 * v1; row[8] = v2; }
        else { row[0] = u1; row[1] = v1; row[2] = 1.f; row[3] = 0.f; row[4] = 0.f; row[5] = 0.f; row[6] = -u2 * u1; row[7] = -u2 * v1; row[8] = -u2; }
        for (int k = 0; k < 9; k++) ws->G[r * 9 + k] = (double)row[k];
    }
    if (WAVE) HS_JACOBI_SYNC();
    hs_jacobi_svd<WAVE>(ws->G, rows, 9, ws->V, ws->sig, ws->perm);
    // vt.row(8): the right singular vector of the smallest singular value, its first component of largest magnitude positive (D20)
    const int c = ws->perm[8];
    double v[9], big = -1.0; bool neg = false;
    for (int k = 0; k < 9; k++) {
        v[k] = ws->V[k * 9 + c];
        if (fabs(v[k]) > big) { big = fabs(v[k]); neg = v[k] < 0.0; }
    }
    float n[9];
    for (int k = 0; k < 9; k++) n[k] = (float)(neg ? -v[k] : v[k]);
    float tmp[9];
    if (model == 0) {
        mono_mul33(prep + 18, n, tmp);
        mono_mul33(tmp, prep, M);
        mono_inv33(M, Minv);
        return;
    }
    HsJacobiSolo<3, 3> s;                                          // Fpre = u diag(w0, w1, 0) vt: the two leading terms of G V^T, one narrowing
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) s.G[i][j] = (double)n[3 * i + j];
    hs_jacobi_solo(s);
    double v0[3], g0[3], v1[3], g1[3], sig;
    hs_solo_column(s, 0, v0, g0, &sig);
    hs_solo_column(s, 1, v1, g1, &sig);
    float Fn[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Fn[3 * i + j] = (float)(g0[i] * v0[j] + g1[i] * v1[j]);
    mono_mul33(prep + 27, Fn, tmp);
    mono_mul33(tmp, prep, M);
    for (int k = 0; k < 9; k++) Minv[k] = 0.f;
}

// ---- CheckHomography (:318-401) and CheckFundamental (:403-481) for one match: the two chi-squares, the source's expressions -----------------
MONO_HD inline void mono_chi(int model, const float* M, const float* Mi, float u1, float v1, float u2, float v2, float invSigmaSquare, float* chi)
{
    if (model == 0) {
        const float w2in1inv = 1.0f / (Mi[6] * u2 + Mi[7] * v2 + Mi[8]);
        const float u2in1 = (Mi[0] * u2 + Mi[1] * v2 + Mi[2]) * w2in1inv;
        const float v2in1 = (Mi[3] * u2 + Mi[4] * v2 + Mi[5]) * w2in1inv;
        const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
        chi[0] = squareDist1 * invSigmaSquare;
        const float w1in2inv = 1.0f / (M[6] * u1 + M[7] * v1 + M[8]);
        const float u1in2 = (M[0] * u1 + M[1] * v1 + M[2]) * w1in2inv;
        const float v1in2 = (M[3] * u1 + M[4] * v1 + M[5]) * w1in2inv;
        const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
        chi[1] = squareDist2 * invSigmaSquare;
    } else {
        const float a2 = M[0] * u1 + M[1] * v1 + M[2];
        const float b2 = M[3] * u1 + M[4] * v1 + M[5];
        const float c2 = M[6] * u1 + M[7] * v1 + M[8];
        const float num2 = a2 * u2 + b2 * v2 + c2;
        const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
        chi[0] = squareDist1 * invSigmaSquare;
        const float a1 = M[0] * u2 + M[3] * v2 + M[6];
        const float b1 = M[1] * u2 + M[4] * v2 + M[7];
        const float c1 = M[2] * u2 + M[5] * v2 + M[8];
        const float num1 = a1 * u1 + b1 * v1 + c1;
        const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
        chi[1] = squareDist2 * invSigmaSquare;
    }
}
// the two additions of one match, first term then second; H accepts and scores at 5.991, F accepts at 3.841 and scores with 5.991 (quirk 3)
MONO_HD inline bool mono_score_add(int model, const float* chi, float* score)
{
    const float th = model == 0 ? 5.991f : 3.841f, thScore = 5.991f;
    bool bIn = true;
    if (chi[0] > th) bIn = false; else *score += thScore - chi[0];
    if (chi[1] > th) bIn = false; else *score += thScore - chi[1];
    return bIn;
}
MONO_HD inline float mono_inv_sigma2(float sigma) { return 1.0f / (sigma * sigma); }

// ---- the motions: ReconstructH (:585-700) and DecomposeE (:923-943) --------------------------------------------------------------------------
MONO_HD inline void mono_k33(const float* k, float* K) { K[0] = k[0]; K[1] = 0.f; K[2] = k[2]; K[3] = 0.f; K[4] = k[1]; K[5] = k[3]; K[6] = 0.f; K[7] = 0.f; K[8] = 1.f; }
// false: the d1/d2, d2/d3 gate (:610)
MONO_HD inline bool mono_motions_h(const float* H21, const float* k, float (*R)[9], float (*t)[3])
{
    float K[9], invK[9], tmp[9], A[9], U[9], w[3], Vt[9];
    mono_k33(k, K);
    mono_inv33(K, invK);
    mono_mul33(invK, H21, tmp);
    mono_mul33(tmp, K, A);
    mono_svd33(A, U, w, Vt);
    const float s = (float)(mono_det33(U) * mono_det33(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return false;      // a NaN ratio passes, as in the source: its motions are NaN and no point is good
    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[4] = { aux1, aux1, -aux1, -aux1 };
    const float x3[4] = { aux3, -aux3, aux3, -aux3 };
    const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float stheta[4] = { aux_stheta, -aux_stheta, -aux_stheta, aux_stheta };
    const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sphi[4] = { aux_sphi, -aux_sphi, -aux_sphi, aux_sphi };
    for (int m = 0; m < 8; m++) {
        const int i = m & 3;
        float Rp[9] = { 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f }, tp[3], M2[9];
        if (m < 4) {
            Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta;
            tp[0] = x1[i] * (d1 - d3); tp[1] = 0.f * (d1 - d3); tp[2] = -x3[i] * (d1 - d3);
        } else {
            Rp[0] = cphi; Rp[2] = sphi[i]; Rp[4] = -1.f; Rp[6] = sphi[i]; Rp[8] = -cphi;
            tp[0] = x1[i] * (d1 + d3); tp[1] = 0.f * (d1 + d3); tp[2] = x3[i] * (d1 + d3);
        }
        mono_mul33(U, Rp, tmp);
        mono_mul33(tmp, Vt, M2);
        for (int e = 0; e < 9; e++) R[m][e] = s * M2[e];
        mono_mul31(U, tp, t[m]);
        mono_unit3(t[m]);
    }
    return true;
}
// the four motions of ReconstructF in its order: (R1, t), (R2, t), (R1, -t), (R2, -t)
MONO_HD inline void mono_motions_f(const float* F21, const float* k, float (*R)[9], float (*t)[3])
{
    float K[9], Kt[9], tmp[9], E[9], u[9], w[3], vt[9], R1[9], R2[9], tt[3];
    mono_k33(k, K);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Kt[3 * i + j] = K[3 * j + i];
    mono_mul33(Kt, F21, tmp);
    mono_mul33(tmp, K, E);
    mono_svd33(E, u, w, vt);
    tt[0] = u[2]; tt[1] = u[5]; tt[2] = u[8];
    mono_unit3(tt);
    const float W[9] = { 0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f }, Wt[9] = { 0.f, 1.f, 0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 1.f };
    mono_mul33(u, W, tmp);
    mono_mul33(tmp, vt, R1);
    if (mono_det33(R1) < 0.0) for (int e = 0; e < 9; e++) R1[e] = -R1[e];
    mono_mul33(u, Wt, tmp);
    mono_mul33(tmp, vt, R2);
    if (mono_det33(R2) < 0.0) for (int e = 0; e < 9; e++) R2[e] = -R2[e];
    for (int m = 0; m < 4; m++) {
        for (int e = 0; e < 9; e++) R[m][e] = (m & 1) ? R2[e] : R1[e];
        for (int e = 0; e < 3; e++) t[m][e] = m < 2 ? tt[e] : -tt[e];
    }
}

// ---- CheckRT (:810-921) ---------------------------------------------------------------------------------------------------------------------------
MONO_HD inline void mono_motion_setup(const float* R, const float* t, const float* k, MonoMotion* m)
{
    float K[9];
    mono_k33(k, K);
    for (int e = 0; e < 9; e++) m->R[e] = R[e];
    for (int e = 0; e < 3; e++) m->t[e] = t[e];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) {
            const float r0 = j < 3 ? R[j] : t[0], r1 = j < 3 ? R[3 + j] : t[1], r2 = j < 3 ? R[6 + j] : t[2];
            m->P2[4 * i + j] = (float)(((double)K[3 * i] * (double)r0 + (double)K[3 * i + 1] * (double)r1) + (double)K[3 * i + 2] * (double)r2);
        }
    for (int i = 0; i < 3; i++) m->O2[i] = -(float)(((double)R[i] * (double)t[0] + (double)R[3 + i] * (double)t[1]) + (double)R[6 + i] * (double)t[2]);
}
// one inlier match: 0 rejected, 1 accepted (its point and cosine count), 2 accepted and good.  X and *cosp are written for 1 and 2.
MONO_HD inline int mono_check_point(const MonoMotion& m, const float* k, float u1, float v1, float u2, float v2, float th2, float* X, float* cosp)
{
    const float P1[12] = { k[0], 0.f, k[2], 0.f, 0.f, k[1], k[3], 0.f, 0.f, 0.f, 1.f, 0.f };
    HsJacobiSolo<4, 4> s;
#pragma unroll
    for (int j = 0; j < 4; j++) {                                  // Triangulate (:746-759): separately rounded float operations
        s.G[0][j] = (double)(u1 * P1[8 + j] - P1[j]);
        s.G[1][j] = (double)(v1 * P1[8 + j] - P1[4 + j]);
        s.G[2][j] = (double)(u2 * m.P2[8 + j] - m.P2[j]);
        s.G[3][j] = (double)(v2 * m.P2[8 + j] - m.P2[4 + j]);
    }
    hs_jacobi_solo(s);
    double v[4], g[4], sig;
    hs_solo_column(s, 3, v, g, &sig);
    const float x3 = (float)v[3];
    X[0] = (float)v[0] / x3; X[1] = (float)v[1] / x3; X[2] = (float)v[2] / x3;
    if (!mono_finite(X[0]) || !mono_finite(X[1]) || !mono_finite(X[2])) return 0;
    const float dist1 = (float)sqrt(((double)X[0] * (double)X[0] + (double)X[1] * (double)X[1]) + (double)X[2] * (double)X[2]);
    const float n2[3] = { X[0] - m.O2[0], X[1] - m.O2[1], X[2] - m.O2[2] };
    const float dist2 = (float)sqrt(((double)n2[0] * (double)n2[0] + (double)n2[1] * (double)n2[1]) + (double)n2[2] * (double)n2[2]);
    const double dot = ((double)X[0] * (double)n2[0] + (double)X[1] * (double)n2[1]) + (double)X[2] * (double)n2[2];
    const float cosParallax = (float)(dot / (double)(dist1 * dist2));
    const bool low = (double)cosParallax < 0.99998;
    if (X[2] <= 0.f && low) return 0;
    float X2[3];
    for (int i = 0; i < 3; i++)
        X2[i] = (float)((((double)m.R[3 * i] * (double)X[0] + (double)m.R[3 * i + 1] * (double)X[1]) + (double)m.R[3 * i + 2] * (double)X[2]) + (double)m.t[i]);
    if (X2[2] <= 0.f && low) return 0;
    const float invZ1 = 1.0f / X[2];
    const float im1x = k[0] * X[0] * invZ1 + k[2], im1y = k[1] * X[1] * invZ1 + k[3];
    const float squareError1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
    if (squareError1 > th2) return 0;
    const float invZ2 = 1.0f / X2[2];
    const float im2x = k[0] * X2[0] * invZ2 + k[2], im2y = k[1] * X2[1] * invZ2 + k[3];
    const float squareError2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
    if (squareError2 > th2) return 0;
    *cosp = cosParallax;
    return low ? 2 : 1;
}
MONO_HD inline float mono_th2(float sigma) { return (float)(4.0 * (double)(sigma * sigma)); }

// ---- the two decisions (:512-582, :702-743) under D21: cosk[m] is the selected cosine of motion m, read only where n_good[m] > 0 ---------------------
// returns the motion to hand out or -1; *decider: the motion that decided, or -1
MONO_HD inline int mono_decide_f(const int* n_good, const float* cosk, int N, int min_tri, float min_frac, float cos_min, int* decider)
{
    int maxGood = n_good[0];
    for (int m = 1; m < 4; m++) if (n_good[m] > maxGood) maxGood = n_good[m];
    const int fracN = (int)(min_frac * (float)N);
    const int nMinGood = fracN > min_tri ? fracN : min_tri;
    int nsimilar = 0;
    for (int m = 0; m < 4; m++) if ((double)n_good[m] > 0.7 * (double)maxGood) nsimilar++;
    *decider = -1;
    if (maxGood < nMinGood || nsimilar > 1) return -1;
    for (int m = 0; m < 4; m++)
        if (maxGood == n_good[m]) {                                // the else-if chain: the first motion equal to the maximum decides alone
            *decider = m;
            return n_good[m] > 0 && cosk[m] < cos_min ? m : -1;    // parallax > minParallax; with nGood == 0 the parallax is 0
        }
    return -1;
}
MONO_HD inline int mono_decide_h(const int* n_good, const float* cosk, int N, int min_tri, float min_frac, float cos_min, int* decider)
{
    int bestGood = 0, secondBestGood = 0, idx = -1;
    for (int m = 0; m < 8; m++) {
        if (n_good[m] > bestGood) { secondBestGood = bestGood; bestGood = n_good[m]; idx = m; }
        else if (n_good[m] > secondBestGood) secondBestGood = n_good[m];
    }
    *decider = idx;
    if (idx < 0) return -1;                                        // bestParallax stays -1
    const bool ok = (double)secondBestGood < 0.75 * (double)bestGood && cosk[idx] <= cos_min && bestGood > min_tri && (float)bestGood > min_frac * (float)N;
    return ok ? idx : -1;
}

#ifndef HS_MONOINIT_MATH_ONLY           // a host program that checks or times the math alone stops here

__global__ __launch_bounds__(1024) void k_mono_prepare(const HsMonoBatch B, const hs_keypoint* __restrict__ kps1, const hs_keypoint* __restrict__ kps2,
                                                       const int32_t* __restrict__ matches12, int32_t* __restrict__ wn, float* __restrict__ wprep,
                                                       int32_t* __restrict__ wm1, int32_t* __restrict__ wm2)
{
    __shared__ uint32_t s_wave[16];
    __shared__ float s_xy[4][HS_MONO_KEY_CHUNK];
    __shared__ float s_mean[4], s_dev[4];
    const HsMonoProblem& p = B.p[blockIdx.x];
    const int tid = threadIdx.x;
    const hs_keypoint* k1 = kps1 + p.off1;
    const hs_keypoint* k2 = kps2 + p.off2;
    // mvMatches12 (:53-65): ascending i
    uint32_t base = 0;
    for (long long i0 = 0; i0 < p.n1; i0 += 1024) {
        const long long i = i0 + tid;
        const int m = i < p.n1 ? matches12[p.off1 + i] : -1;
        const uint32_t keep = (unsigned)m < (unsigned)p.n2 ? 1u : 0u;
        uint32_t total;
        const uint32_t pos = base + block_scan_excl(keep, s_wave, total);
        if (keep) { wm1[p.off1 + pos] = (int)i; wm2[p.off1 + pos] = m; }
        base += total;
        __syncthreads();                                           // s_wave is rewritten by the next chunk
    }
    if (tid == 0) wn[p.q] = (int)base;
    // Normalize (:761-807) over ALL key points of each frame (quirk 1): chain `tid` < 4 is x1, y1, x2, y2
    const int nmax = p.n1 > p.n2 ? p.n1 : p.n2;
    const int nn = tid < 2 ? p.n1 : p.n2;
    for (int pass = 0; pass < 2; pass++) {
        float acc = 0.f;
        const float mean = pass == 1 && tid < 4 ? s_mean[tid] : 0.f;
        for (long long c0 = 0; c0 < nmax; c0 += HS_MONO_KEY_CHUNK) {
            __syncthreads();
            const long long i = c0 + tid;
            if (i < p.n1) { s_xy[0][tid] = k1[i].x; s_xy[1][tid] = k1[i].y; }
            if (i < p.n2) { s_xy[2][tid] = k2[i].x; s_xy[3][tid] = k2[i].y; }
            __syncthreads();
            if (tid < 4) {
                const long long left = (long long)nn - c0;
                const int m = left < 0 ? 0 : left < HS_MONO_KEY_CHUNK ? (int)left : HS_MONO_KEY_CHUNK;
                if (pass == 0) for (int j = 0; j < m; j++) acc += s_xy[tid][j];
                else for (int j = 0; j < m; j++) acc += fabsf(s_xy[tid][j] - mean);
            }
        }
        if (tid < 4) { if (pass == 0) s_mean[tid] = acc / nn; else s_dev[tid] = acc / nn; }
        __syncthreads();
    }
    if (tid == 0) {
        float prep[HS_MONO_PREP_WORDS];
        mono_prep(s_mean, s_dev, prep);
        for (int i = 0; i < HS_MONO_PREP_WORDS; i++) wprep[(size_t)p.q * HS_MONO_PREP_WORDS + i] = prep[i];
    }
}

__global__ __launch_bounds__(64) void k_mono_hypotheses(const HsMonoBatch B, const hs_keypoint* __restrict__ kps1, const hs_keypoint* __restrict__ kps2,
                                                        const uint32_t* __restrict__ draws, int draw_cap, int H, const int32_t* __restrict__ wn,
                                                        const float* __restrict__ wprep, const int32_t* __restrict__ wm1, const int32_t* __restrict__ wm2,
                                                        float* __restrict__ wscore, float* __restrict__ wmodel)
{
    __shared__ MonoWs ws;
    __shared__ float s_chi[2 * HS_MONO_CHI_CHUNK];
    __shared__ float s_prep[HS_MONO_PREP_WORDS];
    const HsMonoProblem& p = B.p[blockIdx.z];
    const int it = blockIdx.x, model = blockIdx.y, lane = threadIdx.x;
    const int n = wn[p.q];
    if (n < 8 || it >= p.max_its) return;                          // the whole workgroup
    if (lane < HS_MONO_PREP_WORDS) s_prep[lane] = wprep[(size_t)p.q * HS_MONO_PREP_WORDS + lane];
    const hs_keypoint* k1 = kps1 + p.off1;
    const hs_keypoint* k2 = kps2 + p.off2;
    const int32_t* m1 = wm1 + p.off1;
    const int32_t* m2 = wm2 + p.off1;
    const MonoSampler sp{ n, p.q, p.seed };
    const int set = 8;
    int smp[8];
    hs_ransac_sample<8, /*WRITE_AT_VALUE=*/false>(sp, set, draws, draw_cap, HS_MONOINIT_DRAW_STRIDE, it, smp);
    __syncthreads();
    float a[8][2], b[8][2];
    for (int j = 0; j < 8; j++) {
        const hs_keypoint ka = k1[m1[smp[j]]], kb = k2[m2[smp[j]]];
        mono_normalized(s_prep, 0, ka.x, ka.y, a[j]);
        mono_normalized(s_prep, 1, kb.x, kb.y, b[j]);
    }
    float M[9], Mi[9];
    mono_hypothesis<true>(model, s_prep, a, b, &ws, M, Mi);
    const float inv_s2 = mono_inv_sigma2(p.sigma);
    float score = 0.f;
    for (long long base = 0; base < n; base += HS_MONO_CHI_CHUNK) {
        const int m = n - base < HS_MONO_CHI_CHUNK ? (int)(n - base) : HS_MONO_CHI_CHUNK;
        __syncthreads();
        for (int i = lane; i < m; i += 64) {
            const hs_keypoint ka = k1[m1[base + i]], kb = k2[m2[base + i]];
            mono_chi(model, M, Mi, ka.x, ka.y, kb.x, kb.y, inv_s2, s_chi + 2 * i);
        }
        __syncthreads();
        if (lane == 0)
            for (int i = 0; i < m; i++) (void)mono_score_add(model, s_chi + 2 * i, &score);
    }
    if (lane < HS_MONO_MODEL_WORDS) {
        const size_t slot = ((size_t)p.q * 2 + (size_t)model) * (size_t)H + (size_t)it;
        if (lane == 0) wscore[slot] = score;
        wmodel[slot * HS_MONO_MODEL_WORDS + lane] = lane < 9 ? M[lane] : 0.f;
    }
}

// The other layout of stage 2: grid (ceil(H / 64), model, problem), one LANE per hypothesis.  A lane owns its hypothesis from the sample to the score
// (the Jacobi on a workspace of its own); the workgroup stages the matches in LDS, HS_MONO_CHI_CHUNK at a time, and every lane walks the chunk in
// match order with its own model: all lanes read the same LDS word at the same time (a broadcast).  The same functions on the same inputs in the same
// order as k_mono_hypotheses: the same bits.  Chosen by hs_debug_monoinit_layout(1); profiles/README.md has the measurement that decided.
__global__ __launch_bounds__(64) void k_mono_hypotheses_lane(const HsMonoBatch B, const hs_keypoint* __restrict__ kps1, const hs_keypoint* __restrict__ kps2,
                                                             const uint32_t* __restrict__ draws, int draw_cap, int H, const int32_t* __restrict__ wn,
                                                             const float* __restrict__ wprep, const int32_t* __restrict__ wm1, const int32_t* __restrict__ wm2,
                                                             float* __restrict__ wscore, float* __restrict__ wmodel)
{
    __shared__ float s_uv[HS_MONO_CHI_CHUNK * 4];
    __shared__ float s_prep[HS_MONO_PREP_WORDS];
    const HsMonoProblem& p = B.p[blockIdx.z];
    const int model = blockIdx.y, lane = threadIdx.x;
    const int it = (int)(blockIdx.x * 64) + lane;
    const int n = wn[p.q];
    if (n < 8 || (int)(blockIdx.x * 64) >= p.max_its) return;      // the whole workgroup
    const bool active = it < p.max_its;
    if (lane < HS_MONO_PREP_WORDS) s_prep[lane] = wprep[(size_t)p.q * HS_MONO_PREP_WORDS + lane];
    const hs_keypoint* k1 = kps1 + p.off1;
    const hs_keypoint* k2 = kps2 + p.off2;
    const int32_t* m1 = wm1 + p.off1;
    const int32_t* m2 = wm2 + p.off1;
    __syncthreads();
    float M[9] = {}, Mi[9] = {};
    if (active) {
        const MonoSampler sp{ n, p.q, p.seed };
        const int set = 8;
        int smp[8];
        hs_ransac_sample<8, /*WRITE_AT_VALUE=*/false>(sp, set, draws, draw_cap, HS_MONOINIT_DRAW_STRIDE, it, smp);
        float a[8][2], b[8][2];
        for (int j = 0; j < 8; j++) {
            const hs_keypoint ka = k1[m1[smp[j]]], kb = k2[m2[smp[j]]];
            mono_normalized(s_prep, 0, ka.x, ka.y, a[j]);
            mono_normalized(s_prep, 1, kb.x, kb.y, b[j]);
        }
        MonoWs ws;
        mono_hypothesis<false>(model, s_prep, a, b, &ws, M, Mi);
    }
    const float inv_s2 = mono_inv_sigma2(p.sigma);
    float score = 0.f;
    for (long long base = 0; base < n; base += HS_MONO_CHI_CHUNK) {
        const int m = n - base < HS_MONO_CHI_CHUNK ? (int)(n - base) : HS_MONO_CHI_CHUNK;
        __syncthreads();
        for (int i = lane; i < m; i += 64) {
            const hs_keypoint ka = k1[m1[base + i]], kb = k2[m2[base + i]];
            s_uv[4 * i] = ka.x; s_uv[4 * i + 1] = ka.y; s_uv[4 * i + 2] = kb.x; s_uv[4 * i + 3] = kb.y;
        }
        __syncthreads();
        if (active)
            for (int i = 0; i < m; i++) {
                float chi[2];
                mono_chi(model, M, Mi, s_uv[4 * i], s_uv[4 * i + 1], s_uv[4 * i + 2], s_uv[4 * i + 3], inv_s2, chi);
                (void)mono_score_add(model, chi, &score);
            }
    }
    if (active) {
        const size_t slot = ((size_t)p.q * 2 + (size_t)model) * (size_t)H + (size_t)it;
        wscore[slot] = score;
        for (int k = 0; k < HS_MONO_MODEL_WORDS; k++) wmodel[slot * HS_MONO_MODEL_WORDS + k] = k < 9 ? M[k] : 0.f;
    }
}

__global__ __launch_bounds__(256) void k_mono_select(const HsMonoBatch B, const hs_keypoint* __restrict__ kps1, const hs_keypoint* __restrict__ kps2, int H,
                                                     const int32_t* __restrict__ wn, const int32_t* __restrict__ wm1, const int32_t* __restrict__ wm2,
                                                     const float* __restrict__ wscore, const float* __restrict__ wmodel, hs_monoinit_result* __restrict__ results,
                                                     uint8_t* __restrict__ inliers_h, uint8_t* __restrict__ inliers_f)
{
    __shared__ float s_s[256];
    __shared__ int s_i[256];
    __shared__ float s_best[2];
    __shared__ int s_it[2];
    const HsMonoProblem& p = B.p[blockIdx.x];
    const int tid = threadIdx.x;
    const int n = wn[p.q];
    const hs_keypoint* k1 = kps1 + p.off1;
    const hs_keypoint* k2 = kps2 + p.off2;
    const int32_t* m1 = wm1 + p.off1;
    const int32_t* m2 = wm2 + p.off1;
    hs_monoinit_result r{};
    r.n_matches = n; r.best_solution = -1; r.best_it_h = -1; r.best_it_f = -1; r.cos_parallax = 1.f;
    if (n < 8) {                                                   // RandomInt(0, -1) in the reference (quirk 7)
        for (long long i = tid; i < p.n1; i += 256) { inliers_h[p.off1 + i] = 0; inliers_f[p.off1 + i] = 0; }
        hs_monoinit_result z{};                                     // everything zero but the count
        z.status = HS_MONOINIT_TOO_FEW; z.n_matches = n;
        if (tid == 0) results[p.q] = z;
        return;
    }
    for (int model = 0; model < 2; model++) {                      // currentScore > score from score = 0 (:178, :229): the first of the largest, never a NaN
        const float* sc = wscore + ((size_t)p.q * 2 + (size_t)model) * (size_t)H;
        float bs = 0.f; int bi = -1;
        for (int it = tid; it < p.max_its; it += 256) { const float s = sc[it]; if (s > bs) { bs = s; bi = it; } }
        s_s[tid] = bs; s_i[tid] = bi;
        __syncthreads();
        if (tid == 0) {
            bs = 0.f; bi = -1;
            for (int t = 0; t < 256; t++)
                if (s_i[t] >= 0 && (s_s[t] > bs || (s_s[t] == bs && s_i[t] < bi))) { bs = s_s[t]; bi = s_i[t]; }
            s_best[model] = bs; s_it[model] = bi;
        }
        __syncthreads();
    }
    const float inv_s2 = mono_inv_sigma2(p.sigma);
    for (int model = 0; model < 2; model++) {
        uint8_t* mask = (model == 0 ? inliers_h : inliers_f) + p.off1;
        float M[9] = {}, Mi[9] = {};
        const int bi = s_it[model];
        if (bi >= 0) {
            const float* src = wmodel + (((size_t)p.q * 2 + (size_t)model) * (size_t)H + (size_t)bi) * HS_MONO_MODEL_WORDS;
            for (int k = 0; k < 9; k++) M[k] = src[k];
            if (model == 0) mono_inv33(M, Mi);
        }
        for (int k = 0; k < 9; k++) (model == 0 ? r.H21 : r.F21)[k] = M[k];
        for (long long i = tid; i < p.n1; i += 256) {
            uint8_t in = 0;
            if (i < n && bi >= 0) {
                const hs_keypoint ka = k1[m1[i]], kb = k2[m2[i]];
                float chi[2], unused = 0.f;
                mono_chi(model, M, Mi, ka.x, ka.y, kb.x, kb.y, inv_s2, chi);
                in = mono_score_add(model, chi, &unused) ? 1 : 0;
            }
            mask[i] = in;                                          // quirk 2: no F hypothesis above 0 leaves an all-zero mask
        }
    }
    if (tid == 0) {
        r.score_h = s_best[0]; r.score_f = s_best[1]; r.best_it_h = s_it[0]; r.best_it_f = s_it[1];
        r.rh = r.score_h / (r.score_h + r.score_f);
        r.model = (double)r.rh > 0.40 ? HS_MONOINIT_MODEL_H : HS_MONOINIT_MODEL_F;           // :129; a NaN goes to F
        if ((r.model == HS_MONOINIT_MODEL_F && r.best_it_f < 0) || (r.model == HS_MONOINIT_MODEL_H && r.best_it_h < 0)) r.model = HS_MONOINIT_MODEL_NONE;
        r.status = HS_MONOINIT_FAILED;
        results[p.q] = r;
    }
}

__global__ __launch_bounds__(256) void k_mono_reconstruct(const HsMonoBatch B, const hs_keypoint* __restrict__ kps1, const hs_keypoint* __restrict__ kps2,
                                                          const int32_t* __restrict__ wn, const int32_t* __restrict__ wm1, const int32_t* __restrict__ wm2,
                                                          float* __restrict__ wcos, hs_monoinit_result* __restrict__ results, const uint8_t* __restrict__ inliers_h,
                                                          const uint8_t* __restrict__ inliers_f, float* __restrict__ p3d, uint8_t* __restrict__ triangulated)
{
    __shared__ float s_R[8][9], s_t[8][3], s_cos[HS_MONO_RANK_CHUNK], s_cosk[8], s_sel;
    __shared__ MonoMotion s_m;
    __shared__ int s_good, s_size, s_N, s_gate, s_ngood[8], s_win, s_dec;
    const HsMonoProblem& p = B.p[blockIdx.x];
    const int tid = threadIdx.x;
    const int n = wn[p.q];
    hs_monoinit_result* res = results + p.q;
    for (long long i = tid; i < p.n1; i += 256) {
        p3d[3 * (p.off1 + i)] = 0.f; p3d[3 * (p.off1 + i) + 1] = 0.f; p3d[3 * (p.off1 + i) + 2] = 0.f;
        triangulated[p.off1 + i] = 0;
    }
    const int model = res->model;
    if (n < 8 || model == HS_MONOINIT_MODEL_NONE) return;         // the whole workgroup; k_mono_select wrote the record
    const hs_keypoint* k1 = kps1 + p.off1;
    const hs_keypoint* k2 = kps2 + p.off2;
    const int32_t* m1 = wm1 + p.off1;
    const int32_t* m2 = wm2 + p.off1;
    const uint8_t* mask = (model == HS_MONOINIT_MODEL_H ? inliers_h : inliers_f) + p.off1;
    float* cosv = wcos + p.off1;
    const int nm = model == HS_MONOINIT_MODEL_H ? 8 : 4;
    const float th2 = mono_th2(p.sigma);
    if (tid == 0) {
        s_N = 0; s_win = -1; s_dec = -1;
        for (int m = 0; m < 8; m++) { s_ngood[m] = 0; s_cosk[m] = 1.f; }
        if (model == HS_MONOINIT_MODEL_H) s_gate = mono_motions_h(res->H21, p.k, s_R, s_t) ? 1 : 0;
        else { mono_motions_f(res->F21, p.k, s_R, s_t); s_gate = 1; }
    }
    __syncthreads();
    if (!s_gate) return;                                           // status stays FAILED
    int cnt = 0;
    for (int i = tid; i < n; i += 256) cnt += mask[i] ? 1 : 0;
    if (cnt) atomicAdd(&s_N, cnt);                                 // an integer count
    for (int m = 0; m < nm; m++) {
        __syncthreads();
        if (tid == 0) { mono_motion_setup(s_R[m], s_t[m], p.k, &s_m); s_good = 0; s_size = 0; s_sel = 1.f; }
        __syncthreads();
        int good = 0, size = 0;
        for (int i = tid; i < n; i += 256) {
            float c = MONO_INF;
            if (mask[i]) {
                const hs_keypoint ka = k1[m1[i]], kb = k2[m2[i]];
                float X[3], cp = 0.f;
                const int code = mono_check_point(s_m, p.k, ka.x, ka.y, kb.x, kb.y, th2, X, &cp);
                if (code > 0) { c = cp; size++; good += code == 2 ? 1 : 0; }
            }
            cosv[i] = c;
        }
        if (size) atomicAdd(&s_size, size);
        if (good) atomicAdd(&s_good, good);
        __syncthreads();
        if (s_good > 0) {                                          // the element of rank min(minTriangulated, size - 1) of the accepted cosines (quirk 5)
            const int rank = p.min_tri < s_size - 1 ? p.min_tri : s_size - 1;
            for (int ib = 0; ib < n; ib += 256) {
                const int i = ib + tid;
                const float ci = i < n ? cosv[i] : MONO_INF;
                int lt = 0, le = 0;
                for (int jb = 0; jb < n; jb += HS_MONO_RANK_CHUNK) {
                    const int mj = n - jb < HS_MONO_RANK_CHUNK ? n - jb : HS_MONO_RANK_CHUNK;
                    __syncthreads();
                    for (int j = tid; j < mj; j += 256) s_cos[j] = cosv[jb + j];
                    __syncthreads();
                    for (int j = 0; j < mj; j++) { const float c = s_cos[j]; lt += c < ci ? 1 : 0; le += c <= ci ? 1 : 0; }
                    if (n - jb <= HS_MONO_RANK_CHUNK) break;
                }
                if (ci < MONO_INF && lt <= rank && rank < le) s_sel = ci;      // every writer holds the same float
                if (n - ib <= 256) break;
            }
        }
        __syncthreads();
        if (tid == 0) { s_ngood[m] = s_good; s_cosk[m] = s_good > 0 ? s_sel : 1.f; }
    }
    __syncthreads();
    if (tid == 0) {
        int dec = -1;
        s_win = model == HS_MONOINIT_MODEL_H ? mono_decide_h(s_ngood, s_cosk, s_N, p.min_tri, p.min_frac, p.cos_min_parallax, &dec)
                                              : mono_decide_f(s_ngood, s_cosk, s_N, p.min_tri, p.min_frac, p.cos_min_parallax, &dec);
        s_dec = dec;
        mono_motion_setup(s_R[s_win < 0 ? 0 : s_win], s_t[s_win < 0 ? 0 : s_win], p.k, &s_m);
    }
    __syncthreads();
    const int win = s_win;
    if (win >= 0)                                                  // vP3D and vbTriangulated of the chosen motion, by key point of frame 1
        for (int i = tid; i < n; i += 256)
            if (mask[i]) {
                const hs_keypoint ka = k1[m1[i]], kb = k2[m2[i]];
                float X[3], cp = 0.f;
                const int code = mono_check_point(s_m, p.k, ka.x, ka.y, kb.x, kb.y, th2, X, &cp);
                if (code > 0) {                                    // also for an accepted point that is not good (quirk 4)
                    float* o = p3d + 3 * (p.off1 + m1[i]);
                    o[0] = X[0]; o[1] = X[1]; o[2] = X[2];
                    if (code == 2) triangulated[p.off1 + m1[i]] = 1;
                }
            }
    if (tid == 0) {
        for (int m = 0; m < 8; m++) res->n_good[m] = s_ngood[m];
        res->best_solution = s_dec;
        res->cos_parallax = s_dec >= 0 ? s_cosk[s_dec] : 1.f;
        if (win >= 0) {
            bool finite = true;
            for (int e = 0; e < 9; e++) { res->R21[e] = s_R[win][e]; finite = finite && mono_finite(s_R[win][e]); }
            for (int e = 0; e < 3; e++) { res->t21[e] = s_t[win][e]; finite = finite && mono_finite(s_t[win][e]); }
            res->n_triangulated = s_ngood[win];
            res->status = !finite ? HS_MONOINIT_NONFINITE : model == HS_MONOINIT_MODEL_H ? HS_MONOINIT_OK_H : HS_MONOINIT_OK_F;
        }
    }
}
#endif
}  // namespace

#ifndef HS_MONOINIT_MATH_ONLY
#include <atomic>
static std::atomic<int> g_mono_layout{ 0 };                       // 0: one wave per hypothesis (k_mono_hypotheses), 1: one lane per hypothesis
extern "C" int hs_debug_monoinit_layout(int layout)
{
    if (layout != 0 && layout != 1) return g_mono_layout.load(std::memory_order_relaxed);
    return g_mono_layout.exchange(layout, std::memory_order_relaxed);
}

int hs_monoinit_call_bound(int Q, const hs_monoinit_params* params)
{
    int H = 1;
    for (int q = 0; q < Q; q++) H = std::max(H, params[q].max_iterations);
    return H;
}

void hs_launch_monoinit(const HsMonoArgs& a, void* d_work, hipStream_t s)
{
    const int H = hs_monoinit_call_bound(a.Q, a.params);
    HsWorkCursor cur(d_work);
    const HsMonoWork w(cur, a.Q, a.key_offsets1[a.Q], H);
    hs_ransac_for_batches(a.Q, HS_MONO_BATCH, [&](int q0, int nb) {
        HsMonoBatch B{};
        int Hb = 1;
        for (int b = 0; b < nb; b++) {
            const int q = q0 + b;
            const hs_monoinit_params& pp = a.params[q];
            HsMonoProblem& o = B.p[b];
            o.off1 = a.key_offsets1[q]; o.off2 = a.key_offsets2[q]; o.seed = pp.seed;
            o.n1 = (int)(a.key_offsets1[q + 1] - a.key_offsets1[q]); o.n2 = (int)(a.key_offsets2[q + 1] - a.key_offsets2[q]);
            o.max_its = pp.max_iterations; o.min_tri = pp.min_triangulated;
            o.k[0] = pp.fx; o.k[1] = pp.fy; o.k[2] = pp.cx; o.k[3] = pp.cy;
            o.sigma = pp.sigma; o.min_frac = pp.min_frac_triangulated;
            o.cos_min_parallax = (float)cos((double)pp.min_parallax_deg * 3.14159265358979323846 / 180.0);      // D21: the one transcendental, on the host
            o.q = q;
            Hb = std::max(Hb, o.max_its);
        }
        hipLaunchKernelGGL(k_mono_prepare, dim3((unsigned)nb), dim3(1024), 0, s, B, a.kps1, a.kps2, a.matches12, w.n, w.prep, w.m1, w.m2);
        if (g_mono_layout.load(std::memory_order_relaxed) == 0)
            hipLaunchKernelGGL(k_mono_hypotheses, dim3((unsigned)Hb, 2u, (unsigned)nb), dim3(64), 0, s, B, a.kps1, a.kps2, a.draws, a.draw_cap, H, w.n, w.prep, w.m1, w.m2,
                               w.score, w.model);
        else
            hipLaunchKernelGGL(k_mono_hypotheses_lane, dim3(((unsigned)Hb + 63u) / 64u, 2u, (unsigned)nb), dim3(64), 0, s, B, a.kps1, a.kps2, a.draws, a.draw_cap, H, w.n,
                               w.prep, w.m1, w.m2, w.score, w.model);
        hipLaunchKernelGGL(k_mono_select, dim3((unsigned)nb), dim3(256), 0, s, B, a.kps1, a.kps2, H, w.n, w.m1, w.m2, w.score, w.model, a.results, a.inliers_h, a.inliers_f);
        hipLaunchKernelGGL(k_mono_reconstruct, dim3((unsigned)nb), dim3(256), 0, s, B, a.kps1, a.kps2, w.n, w.m1, w.m2, w.cosv, a.results, a.inliers_h, a.inliers_f, a.p3d,
                           a.triangulated);
    });
}
#endif
