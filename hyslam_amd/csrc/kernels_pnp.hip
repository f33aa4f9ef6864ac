// kernels_pnp.hip — batched EPnP RANSAC (PnPsolver, src/estimators/PnPsolver.cc).
//   k_pnp_hypotheses   grid (hypotheses, problems), one wave per hypothesis: the sample of absolute iteration `it` (swap-with-back draws), EPnP on
//                      its min_set points, CheckInliers over all N; writes the count and the twelve doubles of R and t
//   k_pnp_select       one wave per problem: walks the counts in order, and for every strict prefix maximum ("record") recomputes its mask from
//                      the stored pose, compacts the inliers and runs Refine() — the same EPnP over the best set, then a recount — until one
//                      refines; writes the state and the result
// EPnP is ONE routine, pnp_epnp, for both: a wave works on a workspace in LDS.  Lanes work over matrix entries and rows; every sum over the points
// is owned by one lane and runs in point order, which is the reference's order, so there is no reduction order to state.  Scalars every lane needs
// (the Jacobi rotation) are computed by every lane from the same LDS words: the same instructions on the same inputs, so control flow stays uniform.
// The serial parts (3x3 and 6xk bookkeeping, Gauss-Newton, qr_solve) run on lane 0 between two barriers.
// fp64 but for what the reference narrows (CheckInliers, Tcw); -ffp-contract=off; no floating-point atomics; every loop has a bound that no input
// changes (HS_PNP_SVD_SWEEPS sweeps, 5 Gauss-Newton steps, `passes` hypotheses); a NaN makes every comparison false and therefore skips a rotation.
// The math is __host__ __device__ with one "lane" on the host, so a host build of this file computes the same bits.
#include "hs_pnp.h"
#include "hs_jacobi.h"
#include <cfloat>
#include <cmath>

static_assert(sizeof(hs_pnp_corr) == 32 && sizeof(hs_pnp_params) == 56 && sizeof(hs_pnp_state) == 72 && sizeof(hs_pnp_result) == 216 && sizeof(hs_pnp_plan_t) == 16,
              "include/hyslam_amd.h states these layouts");

// the one decomposition is hs_jacobi.h's, under the names this file has always used
#define PNP_LANE HS_JACOBI_LANE
#define PNP_LANES HS_JACOBI_LANES
#define PNP_SYNC() HS_JACOBI_SYNC()
#define PNP_HD HS_JACOBI_HD
#define HS_PNP_SVD_SWEEPS HS_JACOBI_SWEEPS
#define pnp_svd hs_jacobi_svd<true>
#define pnp_cut hs_jacobi_cut
#define PNP_LDS_POINTS 1024              // k_pnp_select keeps the compacted inliers of a problem of at most this many correspondences in LDS (40 KB)

namespace {

struct PnpCam { double fu, fv, uc, vc; };

// a wave's workspace (LDS on the device).  A point is five doubles: Xw, Yw, Zw, u, v.
struct PnpWs {
    double g12[144], v12[144];          // MtM, then its Jacobi image; the right singular vectors; after the sort g12 holds `ut` (row r = vector of rank r)
    double cws[12], ccs[12];            // control points, world and camera
    double g3[9], v3[9], cc_inv[9];     // the 3x3 uses: PCA, the inverse, ABt
    double l610[60], rho[6];
    double lsg[30], lsv[25];            // the 6xk least squares
    double sig[12];                     // singular values by COLUMN; perm[rank] = column
    double Rs[4][9], ts[4][3], rep[4];
    double pc0[3], pw0[3];
    double pts[HS_PNP_MAX_SET * 5];     // the sample of a hypothesis
    double R[9], t[3];                  // compute_pose's answer
    int perm[12];
};

// x = pinv(A) b from the image of pnp_svd (lane 0)
PNP_HD void pnp_pinv_solve(const double* G, int m, int n, const double* V, const double* sig, const int* perm, const double* b, double* x)
{
    const double cut = pnp_cut(sig, perm, n);
    for (int i = 0; i < n; i++) x[i] = 0.0;
    for (int r = 0; r < n; r++) {
        const int c = perm[r];
        if (!(sig[c] > cut)) continue;
        double d = 0.0;
        for (int j = 0; j < m; j++) d = d + (G[j * n + c] / sig[c]) * b[j];
        for (int i = 0; i < n; i++) x[i] = x[i] + V[i * n + c] * (d / sig[c]);
    }
}

PNP_HD void pnp_alphas(const PnpWs* w, const double* pi, double* a)
{
    const double* ci = w->cc_inv;
    const double d0 = pi[0] - w->cws[0], d1 = pi[1] - w->cws[1], d2 = pi[2] - w->cws[2];
    for (int j = 0; j < 3; j++) a[1 + j] = ci[3 * j] * d0 + ci[3 * j + 1] * d1 + ci[3 * j + 2] * d2;
    a[0] = 1.0 - a[1] - a[2] - a[3];
}
// fill_M: entry `c` of the two rows of a point
PNP_HD void pnp_m_entry(const double* a, int c, const PnpCam& cam, double u, double v, double* m1, double* m2)
{
    const int k = c / 3, j = c % 3;
    *m1 = j == 0 ? a[k] * cam.fu : j == 1 ? 0.0 : a[k] * (cam.uc - u);
    *m2 = j == 0 ? 0.0 : j == 1 ? a[k] * cam.fv : a[k] * (cam.vc - v);
}
PNP_HD double pnp_dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
PNP_HD double pnp_dist2(const double* p1, const double* p2)
{
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}
PNP_HD void pnp_pc(const PnpWs* w, const double* pi, double* pc)
{
    double a[4];
    pnp_alphas(w, pi, a);
    for (int j = 0; j < 3; j++) pc[j] = a[0] * w->ccs[j] + a[1] * w->ccs[3 + j] + a[2] * w->ccs[6 + j] + a[3] * w->ccs[9 + j];
}

// qr_solve (:866-956) for the 6x4 system of a Gauss-Newton step; leaves X alone when a column is zero (lane 0)
PNP_HD void pnp_qr_solve(double* pA, double* pb, double* pX)
{
    const int nr = 6, nc = 4;
    double A1[4], A2[4];
    for (int k = 0; k < nc; k++) {
        double* ppAkk = pA + k * (nc + 1);
        double* ppAik = ppAkk;
        double eta = fabs(*ppAik);
        for (int i = k + 1; i < nr; i++) {                         // as written: the element is read before the pointer moves
            const double elt = fabs(*ppAik);
            if (eta < elt) eta = elt;
            ppAik += nc;
        }
        if (eta == 0) return;
        ppAik = ppAkk;
        double sum = 0.0;
        const double inv_eta = 1. / eta;
        for (int i = k; i < nr; i++) { *ppAik *= inv_eta; sum += *ppAik * *ppAik; ppAik += nc; }
        double sigma = sqrt(sum);
        if (*ppAkk < 0) sigma = -sigma;
        *ppAkk += sigma;
        A1[k] = sigma * *ppAkk;
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; j++) {
            double* pp = ppAkk;
            double s2 = 0;
            for (int i = k; i < nr; i++) { s2 += *pp * pp[j - k]; pp += nc; }
            const double tau = s2 / A1[k];
            pp = ppAkk;
            for (int i = k; i < nr; i++) { pp[j - k] -= tau * *pp; pp += nc; }
        }
    }
    for (int j = 0; j < nc; j++) {                                 // b <- Qt b
        double* ppAjj = pA + j * (nc + 1);
        double* pp = ppAjj;
        double tau = 0;
        for (int i = j; i < nr; i++) { tau += *pp * pb[i]; pp += nc; }
        tau /= A1[j];
        pp = ppAjj;
        for (int i = j; i < nr; i++) { pb[i] -= tau * *pp; pp += nc; }
    }
    pX[nc - 1] = pb[nc - 1] / A2[nc - 1];                          // X = R-1 b
    for (int i = nc - 2; i >= 0; i--) {
        const double* pp = pA + i * nc + (i + 1);
        double sum = 0;
        for (int j = i + 1; j < nc; j++) { sum += *pp * pX[j]; pp++; }
        pX[i] = (pb[i] - sum) / A2[i];
    }
}

// gauss_newton (:846-864): 5 steps; x starts at zero (the reference leaves it unset before the first qr_solve)
PNP_HD void pnp_gauss_newton(const double* l, const double* rho, double* betas, double* A /*[24]*/, double* b /*[10]*/)
{
    double* x = b + 6;
    for (int i = 0; i < 4; i++) x[i] = 0.0;
    for (int k = 0; k < 5; k++) {
        for (int i = 0; i < 6; i++) {
            const double* rowL = l + i * 10;
            double* rowA = A + i * 4;
            rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
            rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
            rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
            rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
            b[i] = rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] + rowL[3] * betas[0] * betas[2] +
                             rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] + rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] +
                             rowL[8] * betas[2] * betas[3] + rowL[9] * betas[3] * betas[3]);
        }
        pnp_qr_solve(A, b, x);
        for (int i = 0; i < 4; i++) betas[i] += x[i];
    }
}

// compute_pose (:483-531) over the n points at P; the answer is w->R, w->t.  Called by every lane of the wave.
PNP_HD void pnp_epnp(PnpWs* w, const double* P, int n, const PnpCam cam)
{
    const int lane = PNP_LANE;
    const double dn = (double)n;
    // choose_control_points
    for (int j = lane; j < 3; j += PNP_LANES) {
        double s = 0.0;
        for (int i = 0; i < n; i++) s = s + P[5 * i + j];
        w->cws[j] = s / dn;
    }
    PNP_SYNC();
    for (int e = lane; e < 9; e += PNP_LANES) {
        const int a = e / 3, b = e % 3;
        double s = 0.0;
        for (int i = 0; i < n; i++) s = s + (P[5 * i + a] - w->cws[a]) * (P[5 * i + b] - w->cws[b]);
        w->g3[e] = s;
    }
    PNP_SYNC();
    pnp_svd(w->g3, 3, 3, w->v3, w->sig, w->perm);
    if (lane == 0) {
        for (int i = 1; i < 4; i++) {
            const int c = w->perm[i - 1];
            const double k = sqrt(w->sig[c] / dn);
            int big = 0;                                           // D17: an axis points where its component of largest magnitude is positive
            for (int j = 1; j < 3; j++) if (fabs(w->v3[j * 3 + c]) > fabs(w->v3[big * 3 + c])) big = j;
            const double sgn = w->v3[big * 3 + c] < 0.0 ? -1.0 : 1.0;
            for (int j = 0; j < 3; j++) w->cws[3 * i + j] = w->cws[j] + k * (sgn * w->v3[j * 3 + c]);
        }
        w->rho[0] = pnp_dist2(w->cws, w->cws + 3); w->rho[1] = pnp_dist2(w->cws, w->cws + 6); w->rho[2] = pnp_dist2(w->cws, w->cws + 9);
        w->rho[3] = pnp_dist2(w->cws + 3, w->cws + 6); w->rho[4] = pnp_dist2(w->cws + 3, w->cws + 9); w->rho[5] = pnp_dist2(w->cws + 6, w->cws + 9);
        for (int i = 0; i < 3; i++)
            for (int j = 1; j < 4; j++) w->g3[3 * i + j - 1] = w->cws[3 * j + i] - w->cws[i];
    }
    PNP_SYNC();
    // compute_barycentric_coordinates: the inverse as a pseudo-inverse
    pnp_svd(w->g3, 3, 3, w->v3, w->sig, w->perm);
    if (lane == 0) {
        const double cut = pnp_cut(w->sig, w->perm, 3);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                double acc = 0.0;
                for (int r = 0; r < 3; r++) {
                    const int c = w->perm[r];
                    if (!(w->sig[c] > cut)) continue;
                    acc = acc + w->v3[i * 3 + c] * ((w->g3[j * 3 + c] / w->sig[c]) / w->sig[c]);
                }
                w->cc_inv[3 * i + j] = acc;
            }
    }
    PNP_SYNC();
    // MtM: entry e is one lane's, summed over the rows of M in order
    for (int e = lane; e < 144; e += PNP_LANES) {
        const int ra = e / 12, rb = e % 12;
        double s = 0.0;
        for (int i = 0; i < n; i++) {
            double al[4], a1, a2, b1, b2;
            pnp_alphas(w, P + 5 * i, al);
            pnp_m_entry(al, ra, cam, P[5 * i + 3], P[5 * i + 4], &a1, &a2);
            pnp_m_entry(al, rb, cam, P[5 * i + 3], P[5 * i + 4], &b1, &b2);
            s = s + a1 * b1;
            s = s + a2 * b2;
        }
        w->g12[e] = s;
    }
    PNP_SYNC();
    pnp_svd(w->g12, 12, 12, w->v12, w->sig, w->perm);
    for (int e = lane; e < 144; e += PNP_LANES) w->g12[e] = w->v12[(e % 12) * 12 + w->perm[e / 12]];      // ut: row r = the right singular vector of rank r
    PNP_SYNC();
    const double* ut = w->g12;
    if (lane == 0) {                                               // compute_L_6x10
        const double* v[4] = { ut + 12 * 11, ut + 12 * 10, ut + 12 * 9, ut + 12 * 8 };
        double (*dv)[6][3] = reinterpret_cast<double (*)[6][3]>(w->v12);      // v12 is free once ut stands in g12
        for (int i = 0; i < 4; i++) {
            int a = 0, b = 1;
            for (int j = 0; j < 6; j++) {
                dv[i][j][0] = v[i][3 * a] - v[i][3 * b];
                dv[i][j][1] = v[i][3 * a + 1] - v[i][3 * b + 1];
                dv[i][j][2] = v[i][3 * a + 2] - v[i][3 * b + 2];
                b++;
                if (b > 3) { a++; b = a + 1; }
            }
        }
        for (int i = 0; i < 6; i++) {
            double* row = w->l610 + 10 * i;
            row[0] = pnp_dot3(dv[0][i], dv[0][i]);
            row[1] = 2.0 * pnp_dot3(dv[0][i], dv[1][i]);
            row[2] = pnp_dot3(dv[1][i], dv[1][i]);
            row[3] = 2.0 * pnp_dot3(dv[0][i], dv[2][i]);
            row[4] = 2.0 * pnp_dot3(dv[1][i], dv[2][i]);
            row[5] = pnp_dot3(dv[2][i], dv[2][i]);
            row[6] = 2.0 * pnp_dot3(dv[0][i], dv[3][i]);
            row[7] = 2.0 * pnp_dot3(dv[1][i], dv[3][i]);
            row[8] = 2.0 * pnp_dot3(dv[2][i], dv[3][i]);
            row[9] = pnp_dot3(dv[3][i], dv[3][i]);
        }
    }
    PNP_SYNC();
    for (int var = 1; var <= 3; var++) {
        const int k = var == 1 ? 4 : var == 2 ? 3 : 5;
        if (lane == 0) {
            const int col1[4] = { 0, 1, 3, 6 };
            for (int i = 0; i < 6; i++)
                for (int j = 0; j < k; j++) w->lsg[i * k + j] = w->l610[10 * i + (var == 1 ? col1[j] : j)];
        }
        PNP_SYNC();
        pnp_svd(w->lsg, 6, k, w->lsv, w->sig, w->perm);
        if (lane == 0) {
            double bb[5], betas[4];
            pnp_pinv_solve(w->lsg, 6, k, w->lsv, w->sig, w->perm, w->rho, bb);
            if (var == 1) {                                        // find_betas_approx_1
                if (bb[0] < 0) { betas[0] = sqrt(-bb[0]); betas[1] = -bb[1] / betas[0]; betas[2] = -bb[2] / betas[0]; betas[3] = -bb[3] / betas[0]; }
                else { betas[0] = sqrt(bb[0]); betas[1] = bb[1] / betas[0]; betas[2] = bb[2] / betas[0]; betas[3] = bb[3] / betas[0]; }
            } else {                                               // find_betas_approx_2 and _3
                if (bb[0] < 0) { betas[0] = sqrt(-bb[0]); betas[1] = (bb[2] < 0) ? sqrt(-bb[2]) : 0.0; }
                else { betas[0] = sqrt(bb[0]); betas[1] = (bb[2] > 0) ? sqrt(bb[2]) : 0.0; }
                if (bb[1] < 0) betas[0] = -betas[0];
                betas[2] = var == 3 ? bb[3] / betas[0] : 0.0;
                betas[3] = 0.0;
            }
            pnp_gauss_newton(w->l610, w->rho, betas, w->lsg, w->lsv);      // the least squares' two arrays are free again
            for (int i = 0; i < 12; i++) w->ccs[i] = 0.0;          // compute_ccs
            for (int i = 0; i < 4; i++) {
                const double* v = ut + 12 * (11 - i);
                for (int j = 0; j < 4; j++)
                    for (int c = 0; c < 3; c++) w->ccs[3 * j + c] += betas[i] * v[3 * j + c];
            }
            double pc[3];                                          // solve_for_sign: pcs[2] only; negating ccs negates every pc exactly
            pnp_pc(w, P, pc);
            if (pc[2] < 0.0)
                for (int i = 0; i < 12; i++) w->ccs[i] = -w->ccs[i];
        }
        PNP_SYNC();
        for (int j = lane; j < 6; j += PNP_LANES) {               // estimate_R_and_t: the two centroids
            double s = 0.0;
            for (int i = 0; i < n; i++) {
                if (j < 3) { double pc[3]; pnp_pc(w, P + 5 * i, pc); s = s + pc[j]; }
                else s = s + P[5 * i + j - 3];
            }
            if (j < 3) w->pc0[j] = s / dn; else w->pw0[j - 3] = s / dn;
        }
        PNP_SYNC();
        for (int e = lane; e < 9; e += PNP_LANES) {
            const int j = e / 3, c = e % 3;
            double s = 0.0;
            for (int i = 0; i < n; i++) {
                double pc[3];
                pnp_pc(w, P + 5 * i, pc);
                s = s + (pc[j] - w->pc0[j]) * (P[5 * i + c] - w->pw0[c]);
            }
            w->g3[e] = s;
        }
        PNP_SYNC();
        pnp_svd(w->g3, 3, 3, w->v3, w->sig, w->perm);
        if (lane == 0) {
            double* R = w->Rs[var];
            double* t = w->ts[var];
            double U[9], Vs[9];
            for (int i = 0; i < 3; i++)
                for (int r = 0; r < 3; r++) { const int c = w->perm[r]; U[3 * i + r] = w->g3[3 * i + c] / w->sig[c]; Vs[3 * i + r] = w->v3[3 * i + c]; }
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) R[3 * i + j] = pnp_dot3(U + 3 * i, Vs + 3 * j);
            const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
            if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
            t[0] = w->pc0[0] - pnp_dot3(R, w->pw0);
            t[1] = w->pc0[1] - pnp_dot3(R + 3, w->pw0);
            t[2] = w->pc0[2] - pnp_dot3(R + 6, w->pw0);
            double sum2 = 0.0;                                     // reprojection_error: a mean of distances
            for (int i = 0; i < n; i++) {
                const double* pw = P + 5 * i;
                const double Xc = pnp_dot3(R, pw) + t[0], Yc = pnp_dot3(R + 3, pw) + t[1], inv_Zc = 1.0 / (pnp_dot3(R + 6, pw) + t[2]);
                const double ue = cam.uc + cam.fu * Xc * inv_Zc, ve = cam.vc + cam.fv * Yc * inv_Zc;
                const double u = pw[3], v = pw[4];
                sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
            }
            w->rep[var] = sum2 / dn;
        }
        PNP_SYNC();
    }
    if (lane == 0) {
        int N = 1;
        if (w->rep[2] < w->rep[1]) N = 2;
        if (w->rep[3] < w->rep[N]) N = 3;
        for (int i = 0; i < 9; i++) w->R[i] = w->Rs[N][i];
        for (int i = 0; i < 3; i++) w->t[i] = w->ts[N][i];
    }
    PNP_SYNC();
}

// CheckInliers (:314-345) for one correspondence, in its mixed precision
PNP_HD bool pnp_inlier(const double* R, const double* t, const PnpCam& cam, const hs_pnp_corr& c, float th2)
{
    const float Xc = (float)(R[0] * c.Xw[0] + R[1] * c.Xw[1] + R[2] * c.Xw[2] + t[0]);
    const float Yc = (float)(R[3] * c.Xw[0] + R[4] * c.Xw[1] + R[5] * c.Xw[2] + t[1]);
    const float invZc = (float)(1 / (R[6] * c.Xw[0] + R[7] * c.Xw[1] + R[8] * c.Xw[2] + t[2]));
    const double ue = cam.uc + cam.fu * Xc * invZc;
    const double ve = cam.vc + cam.fv * Yc * invZc;
    const float distX = (float)(c.u - ue);
    const float distY = (float)(c.v - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < c.sigma2 * th2;
}

// the sample of absolute iteration `it` (:194-207): min_set draws, swap-with-back (hs_ransac.h).  n >= min_inliers >= min_set.
PNP_HD void pnp_sample(const HsPnpProblem& p, long long it, const uint32_t* draws, int draw_cap, int* sample)
{
    hs_ransac_sample<HS_PNP_MAX_SET, /*WRITE_AT_VALUE=*/false>(p, p.min_set, draws, draw_cap, HS_PNP_MAX_SET, it, sample);
}

__device__ __forceinline__ PnpCam pnp_cam(const HsPnpProblem& p) { return PnpCam{ (double)p.fx, (double)p.fy, (double)p.cx, (double)p.cy }; }
__device__ __forceinline__ void pnp_load_point(const hs_pnp_corr& c, double* dst)
{
    dst[0] = (double)c.Xw[0]; dst[1] = (double)c.Xw[1]; dst[2] = (double)c.Xw[2]; dst[3] = (double)c.u; dst[4] = (double)c.v;
}
// the wave's count of inliers over the problem's correspondences; mask (may be nullptr) receives the flags
__device__ int pnp_count(const double* R, const double* t, const PnpCam& cam, const hs_pnp_corr* corrs, int n, float th2, uint8_t* mask, int* s_cnt)
{
    if (threadIdx.x == 0) *s_cnt = 0;
    __syncthreads();
    int local = 0;
    for (int i = threadIdx.x; i < n; i += 64) {
        const bool in = pnp_inlier(R, t, cam, corrs[i], th2);
        if (mask) mask[i] = in ? 1 : 0;
        local += in ? 1 : 0;
    }
    atomicAdd(s_cnt, local);                                       // integers: the order does not show
    __syncthreads();
    const int c = *s_cnt;
    __syncthreads();
    return c;
}

__global__ __launch_bounds__(64) void k_pnp_hypotheses(const HsPnpBatch B, const hs_pnp_corr* __restrict__ corrs, int n_iterations, const uint32_t* __restrict__ draws,
                                                       int draw_cap, const hs_pnp_state* __restrict__ states, int H, int32_t* __restrict__ hyp_count,
                                                       double* __restrict__ hyp_pose)
{
    __shared__ PnpWs ws;
    __shared__ int s_sample[HS_PNP_MAX_SET];
    __shared__ int s_cnt;
    const HsPnpProblem& p = B.p[blockIdx.y];
    if (p.n < p.min_inliers) return;
    const int it0 = hs_ransac_it0(states[p.q].iterations);
    const int j = blockIdx.x;
    if (j >= hs_ransac_passes_or(it0, p.max_its, n_iterations, H)) return;
    const hs_pnp_corr* pc = corrs + p.off;
    if (threadIdx.x == 0) pnp_sample(p, (long long)it0 + j, draws, draw_cap, s_sample);
    __syncthreads();
    if ((int)threadIdx.x < p.min_set) pnp_load_point(pc[s_sample[threadIdx.x]], ws.pts + 5 * threadIdx.x);
    __syncthreads();
    const PnpCam cam = pnp_cam(p);
    pnp_epnp(&ws, ws.pts, p.min_set, cam);
    const int cnt = pnp_count(ws.R, ws.t, cam, pc, p.n, p.th2, nullptr, &s_cnt);
    const size_t slot = (size_t)p.q * (size_t)H + (size_t)j;
    if (threadIdx.x == 0) hyp_count[slot] = cnt;
    if (threadIdx.x < 9) hyp_pose[slot * 12 + threadIdx.x] = ws.R[threadIdx.x];
    else if (threadIdx.x < 12) hyp_pose[slot * 12 + threadIdx.x] = ws.t[threadIdx.x - 9];
}

__device__ void pnp_write_pose(hs_pnp_result* r, const double* R, const double* t)
{
    for (int i = 0; i < 16; i++) r->Tcw_d[i] = (i == 15) ? 1.0 : 0.0;
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) r->Tcw_d[4 * i + j] = R[3 * i + j]; r->Tcw_d[4 * i + 3] = t[i]; }
    for (int i = 0; i < 16; i++) r->Tcw[i] = (float)r->Tcw_d[i];
}
__device__ void pnp_finish(hs_pnp_result* r, int status, int n_inliers, int at, int iterations, int hyps, int refines)
{
    bool finite = true;
    for (int i = 0; i < 16; i++) finite = finite && isfinite(r->Tcw_d[i]) && isfinite(r->Tcw[i]);
    r->status = (status == HS_PNP_REFINED || status == HS_PNP_BEST) && !finite ? HS_PNP_NONFINITE : status;
    r->n_inliers = n_inliers; r->at_iteration = at; r->iterations = iterations; r->hypotheses_run = hyps; r->refines_run = refines;
}

__global__ __launch_bounds__(64) void k_pnp_select(const HsPnpBatch B, const hs_pnp_corr* __restrict__ corrs, int n_iterations, hs_pnp_state* __restrict__ states,
                                                   uint8_t* __restrict__ best_masks, hs_pnp_result* __restrict__ results, uint8_t* __restrict__ inlier_masks, int H,
                                                   const int32_t* __restrict__ hyp_count, const double* __restrict__ hyp_pose, double* __restrict__ pts_all,
                                                   uint8_t* __restrict__ tmp_all)
{
    __shared__ PnpWs ws;
    __shared__ int s_cnt;
    __shared__ double s_pose[12];
    __shared__ double s_pts[PNP_LDS_POINTS * 5];
    const HsPnpProblem& p = B.p[blockIdx.x];
    const int lane = threadIdx.x;
    hs_pnp_state* st = states + p.q;
    hs_pnp_result* res = results + p.q;
    if (p.n < p.min_inliers) {
        if (lane == 0) {
            for (int i = 0; i < 16; i++) { res->Tcw_d[i] = 0.0; res->Tcw[i] = 0.f; }
            pnp_finish(res, HS_PNP_TOO_FEW, 0, 0, st->iterations, 0, 0);
        }
        return;
    }
    const hs_pnp_corr* pc = corrs + p.off;
    uint8_t* best_mask = best_masks + p.off;
    uint8_t* out_mask = inlier_masks + p.off;
    uint8_t* tmp_mask = tmp_all + p.off;
    // the refine's points: in LDS when the problem's N fits (every loop over the points is then an LDS read, not a trip to memory), else in the work area
    double* pts = p.n <= PNP_LDS_POINTS ? s_pts : pts_all + 5 * (size_t)p.off;
    const PnpCam cam = pnp_cam(p);
    const int it0 = hs_ransac_it0(st->iterations);
    const int passes = hs_ransac_passes_or(it0, p.max_its, n_iterations, H);
    int best = st->best_inliers;
    int eval = 0, refined_cnt = 0, refines = 0, record = -1;     // eval of the current best set: 0 not yet, 1 Refine() failed, 2 succeeded
    __syncthreads();                                              // the state is read before lane 0 writes it
    for (int j = 0; j < passes; j++) {
        const size_t slot = (size_t)p.q * (size_t)H + (size_t)j;
        const int c = hyp_count[slot];
        if (c < p.min_inliers) continue;
        if (c > best) {                                            // a record: its mask from the stored pose gives the same bits as the count did
            best = c; record = j; eval = 0;
            if (lane < 12) s_pose[lane] = hyp_pose[slot * 12 + lane];
            __syncthreads();
            (void)pnp_count(s_pose, s_pose + 9, cam, pc, p.n, p.th2, best_mask, &s_cnt);
            if (lane == 0) {
                for (int i = 0; i < 16; i++) st->best_Tcw[i] = (i == 15) ? 1.f : 0.f;
                for (int i = 0; i < 3; i++) { for (int k = 0; k < 3; k++) st->best_Tcw[4 * i + k] = (float)s_pose[3 * i + k]; st->best_Tcw[4 * i + 3] = (float)s_pose[9 + i]; }
            }
        }
        if (eval == 0) {                                           // Refine() (:266-311): a pure function of the best set, evaluated once per set
            __syncthreads();
            int n_in = 0;
            for (long long i0 = 0; i0 < p.n; i0 += 64) {          // the inliers in ascending order
                const long long i = i0 + lane;
                const bool f = i < p.n && best_mask[i] != 0;
                const unsigned long long bal = __ballot(f);
                if (f) pnp_load_point(pc[i], pts + 5 * (size_t)(n_in + __popcll(bal & ((1ull << lane) - 1ull))));
                n_in += __popcll(bal);
            }
            __syncthreads();
            pnp_epnp(&ws, pts, n_in, cam);
            refined_cnt = pnp_count(ws.R, ws.t, cam, pc, p.n, p.th2, tmp_mask, &s_cnt);
            refines++;
            eval = refined_cnt > p.min_inliers ? 2 : 1;
        }
        if (eval == 2) {
            __syncthreads();
            for (int i = lane; i < p.n; i += 64) out_mask[i] = tmp_mask[i];
            if (lane == 0) {
                pnp_write_pose(res, ws.R, ws.t);
                pnp_finish(res, HS_PNP_REFINED, refined_cnt, it0 + j + 1, it0 + j + 1, passes, refines);
                st->iterations = it0 + j + 1; st->best_inliers = best;
            }
            return;
        }
    }
    __syncthreads();
    if (best >= p.min_inliers)
        for (int i = lane; i < p.n; i += 64) out_mask[i] = best_mask[i];
    if (lane == 0) {
        st->iterations = it0 + passes; st->best_inliers = best;
        if (best >= p.min_inliers) {
            if (record >= 0) pnp_write_pose(res, s_pose, s_pose + 9);
            for (int i = 0; i < 16; i++) { res->Tcw[i] = st->best_Tcw[i]; if (record < 0) res->Tcw_d[i] = (double)st->best_Tcw[i]; }
            pnp_finish(res, HS_PNP_BEST, best, 0, it0 + passes, passes, refines);
        } else {
            for (int i = 0; i < 16; i++) { res->Tcw_d[i] = 0.0; res->Tcw[i] = 0.f; }
            pnp_finish(res, HS_PNP_NONE, 0, 0, it0 + passes, passes, refines);
        }
    }
}
}  // namespace

int hs_pnp_call_bound(int Q, const hs_pnp_params* params, const int64_t* corr_offsets, int n_iterations)
{
    int H = n_iterations;
    for (int q = 0; q < Q; q++) {
        hs_pnp_plan_t plan;
        if (hs_pnp_plan((int)(corr_offsets[q + 1] - corr_offsets[q]), &params[q], &plan) == HS_OK) H = hs_ransac_passes_or(0, plan.max_iterations, H, INT_MAX);
    }
    return H;
}

void hs_launch_pnp_iterate(const HsPnpArgs& a, void* d_work, hipStream_t s)
{
    const int H = hs_pnp_call_bound(a.Q, a.params, a.corr_offsets, a.n_iterations);
    HsWorkCursor cur(d_work);
    const HsPnpWork w(cur, a.Q, a.corr_offsets[a.Q], H);
    hs_ransac_for_batches(a.Q, HS_PNP_BATCH, [&](int q0, int nb) {
        HsPnpBatch B{};
        for (int b = 0; b < nb; b++) {
            const int q = q0 + b;
            const hs_pnp_params& pp = a.params[q];
            hs_pnp_plan_t plan;
            HsPnpProblem& o = B.p[b];
            o.off = a.corr_offsets[q]; o.n = (int)(a.corr_offsets[q + 1] - a.corr_offsets[q]); o.seed = pp.seed; o.min_set = pp.min_set;
            (void)hs_pnp_plan(o.n, &pp, &plan);
            o.min_inliers = plan.min_inliers; o.max_its = plan.max_iterations;
            o.th2 = pp.th2; o.fx = pp.fx; o.fy = pp.fy; o.cx = pp.cx; o.cy = pp.cy; o.q = q;
        }
        hipLaunchKernelGGL(k_pnp_hypotheses, dim3((unsigned)H, (unsigned)nb), dim3(64), 0, s, B, a.corrs, a.n_iterations, a.draws, a.draw_cap, a.states, H, w.hyp_count,
                           w.hyp_pose);
        hipLaunchKernelGGL(k_pnp_select, dim3((unsigned)nb), dim3(64), 0, s, B, a.corrs, a.n_iterations, a.states, a.best_masks, a.results, a.inlier_masks, H, w.hyp_count,
                           w.hyp_pose, w.pts, w.tmp_mask);
    });
}
