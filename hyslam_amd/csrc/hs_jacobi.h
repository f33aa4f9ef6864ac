// hs_jacobi.h — the one decomposition of the library, shared by the estimators that need an SVD on the device (kernels_pnp.hip: EPnP;
// kernels_monoinit.hip: the null vectors, the 3x3 factorisations and the 4x4 triangulations of MonoEstimator).  Two forms of the same
// one-sided cyclic Jacobi, the same operations in the same order:
//   hs_jacobi_svd<WAVE>  true: a WAVE works on G and V in LDS (lanes over rows), one "lane" on the host; false: one lane on memory of its own
//   hs_jacobi_solo<M,N>  ONE lane owns a small G and V in registers; the dimensions are compile-time so that no array is indexed by a variable
// Plain __host__ __device__ code: + - x / sqrt in double, -ffp-contract=off, HS_JACOBI_SWEEPS sweeps at most; a NaN makes every comparison false and
// therefore skips a rotation.
#pragma once
#include "hs_internal.h"
#include <cfloat>
#include <cmath>

#if defined(__HIP_DEVICE_COMPILE__)
#define HS_JACOBI_LANE ((int)threadIdx.x)
#define HS_JACOBI_LANES 64
#define HS_JACOBI_SYNC() __syncthreads()
#else
#define HS_JACOBI_LANE 0
#define HS_JACOBI_LANES 1
#define HS_JACOBI_SYNC() ((void)0)
#endif
#define HS_JACOBI_HD __host__ __device__
#define HS_JACOBI_SWEEPS 30             // cap on the sweeps of the one-sided Jacobi SVD

namespace {

// ---- the one decomposition: one-sided cyclic Jacobi SVD of G (m x n, row-major), G <- U Sigma, V accumulated -----------------
// WAVE: the 64 lanes of a workgroup work on G and V in LDS (every lane calls it); !WAVE: the calling lane alone, on memory of its own
template <bool WAVE> HS_JACOBI_HD void hs_jacobi_svd(double* G, int m, int n, double* V, double* sig, int* perm)
{
    const int lane = WAVE ? HS_JACOBI_LANE : 0;
    for (int e = lane; e < n * n; e += (WAVE ? HS_JACOBI_LANES : 1)) V[e] = (e / n == e % n) ? 1.0 : 0.0;
    double f2 = 0.0;
    for (int e = 0; e < m * n; e++) f2 = f2 + G[e] * G[e];
    const double tiny = ((double)n * DBL_EPSILON) * ((double)n * DBL_EPSILON) * f2;
    if (WAVE) HS_JACOBI_SYNC();
    for (int sweep = 0; sweep < HS_JACOBI_SWEEPS; sweep++) {
        bool rotated = false;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                double a = 0.0, b = 0.0, g = 0.0;
                for (int i = 0; i < m; i++) {
                    const double gp = G[i * n + p], gq = G[i * n + q];
                    a = a + gp * gp; b = b + gq * gq; g = g + gp * gq;
                }
                if (!(a > tiny) || !(b > tiny) || !(fabs(g) > DBL_EPSILON * sqrt(a * b))) continue;      // the same decision in every lane
                const double zeta = (b - a) / (2.0 * g);
                const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                if (WAVE) HS_JACOBI_SYNC();                                       // every lane has read the two columns
                for (int r = lane; r < m + n; r += (WAVE ? HS_JACOBI_LANES : 1)) {
                    double* row = r < m ? G + r * n : V + (r - m) * n;
                    const double x = row[p], y = row[q];
                    row[p] = c * x - s * y; row[q] = s * x + c * y;
                }
                if (WAVE) HS_JACOBI_SYNC();
                rotated = true;
            }
        if (!rotated) break;
    }
    if (lane == 0) {
        for (int j = 0; j < n; j++) {
            double s = 0.0;
            for (int i = 0; i < m; i++) s = s + G[i * n + j] * G[i * n + j];
            sig[j] = sqrt(s);
        }
        for (int j = 0; j < n; j++) {                              // stable insertion sort, descending
            int k = j;
            while (k > 0 && sig[perm[k - 1]] < sig[j]) { perm[k] = perm[k - 1]; k--; }
            perm[k] = j;
        }
    }
    if (WAVE) HS_JACOBI_SYNC();
}
HS_JACOBI_HD double hs_jacobi_cut(const double* sig, const int* perm, int n)
{
    double s = 0.0;
    for (int r = 0; r < n; r++) s = s + sig[perm[r]];
    return 2.0 * DBL_EPSILON * s;
}

// the same decomposition owned by ONE lane: every loop bound is a compile-time constant and is unrolled, so G and V stay in registers
template <int M, int N> struct HsJacobiSolo { double G[M][N], V[N][N], sig[N]; int perm[N]; };
template <int M, int N> HS_JACOBI_HD inline void hs_jacobi_solo(HsJacobiSolo<M, N>& w)
{
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) w.V[i][j] = i == j ? 1.0 : 0.0;
    double f2 = 0.0;
#pragma unroll
    for (int i = 0; i < M; i++)
#pragma unroll
        for (int j = 0; j < N; j++) f2 = f2 + w.G[i][j] * w.G[i][j];
    const double tiny = ((double)N * DBL_EPSILON) * ((double)N * DBL_EPSILON) * f2;
    for (int sweep = 0; sweep < HS_JACOBI_SWEEPS; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < N - 1; p++)
#pragma unroll
            for (int q = p + 1; q < N; q++) {
                double a = 0.0, b = 0.0, g = 0.0;
#pragma unroll
                for (int i = 0; i < M; i++) {
                    const double gp = w.G[i][p], gq = w.G[i][q];
                    a = a + gp * gp; b = b + gq * gq; g = g + gp * gq;
                }
                if (!(a > tiny) || !(b > tiny) || !(fabs(g) > DBL_EPSILON * sqrt(a * b))) continue;
                const double zeta = (b - a) / (2.0 * g);
                const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                for (int r = 0; r < M; r++) {
                    const double x = w.G[r][p], y = w.G[r][q];
                    w.G[r][p] = c * x - s * y; w.G[r][q] = s * x + c * y;
                }
#pragma unroll
                for (int r = 0; r < N; r++) {
                    const double x = w.V[r][p], y = w.V[r][q];
                    w.V[r][p] = c * x - s * y; w.V[r][q] = s * x + c * y;
                }
                rotated = true;
            }
        if (!rotated) break;
    }
#pragma unroll
    for (int j = 0; j < N; j++) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < M; i++) s = s + w.G[i][j] * w.G[i][j];
        w.sig[j] = sqrt(s);
    }
    // rank of column j, descending and stable: the columns before it that are not smaller and the columns after it that are larger — the place the
    // insertion sort of hs_jacobi_svd gives it
#pragma unroll
    for (int j = 0; j < N; j++) {
        int rank = 0;
#pragma unroll
        for (int k = 0; k < N; k++) rank += (k < j && !(w.sig[k] < w.sig[j])) || (k > j && w.sig[j] < w.sig[k]) ? 1 : 0;
#pragma unroll
        for (int r = 0; r < N; r++) if (r == rank) w.perm[r] = j;
    }
}
// column perm[rank] of V and of G = U Sigma, and its singular value, picked by comparisons so that no register array is indexed by a variable
template <int M, int N> HS_JACOBI_HD inline void hs_solo_column(const HsJacobiSolo<M, N>& w, int rank, double* v /*[N]*/, double* g /*[M]*/, double* sig)
{
    int col = 0;
#pragma unroll
    for (int r = 0; r < N; r++) if (r == rank) col = w.perm[r];
#pragma unroll
    for (int c = 0; c < N; c++)
        if (c == col) {
#pragma unroll
            for (int k = 0; k < N; k++) v[k] = w.V[k][c];
#pragma unroll
            for (int k = 0; k < M; k++) g[k] = w.G[k][c];
            *sig = w.sig[c];
        }
}

}  // namespace
