// kernels_poseopt.hip — Optimizer::PoseOptimization (src/optimizers/Optimizer.cc:48-279) with the parts of g2o it runs through: one 6-DoF vertex, unary
// mono / stereo reprojection edges, Huber, Levenberg-Marquardt, four rounds of optimise-and-classify (entry points: hs_poseopt.hip; the list of what
// "the same result" means: DESIGN.md 5.11, D13, D14).
//
//   k_pose_optimize   ONE launch, one workgroup of HS_POSE_THREADS per problem, the whole 4 x 10 x 10 schedule inside it.  Lanes stride over the
//                     problem's edges; edge e always belongs to lane e % HS_POSE_THREADS, so the outlier flag a lane reads is one it wrote itself.
//                     A pass over the edges is one of three kinds — errors + chi, errors + Jacobians + the 21 upper entries of H + b + chi,
//                     classification — and ends in po_block_sum: a butterfly over the wave, then the waves' partial sums through LDS, added in
//                     wave order by every thread.  After it every thread holds the same bits, so every thread runs the 6x6 LDL^T, exp, the
//                     quaternion product and the lambda bookkeeping on them (the same instructions on the same inputs: the same result in every
//                     lane, and control flow stays uniform without a broadcast or a flag in LDS).
//   k_pose_edges      the edge list of Optimizer.cc:94-188 from resident keypoints, associations and landmarks, compacted in ascending keypoint index
//                     by one workgroup: chunks of 1024 keypoints, block_scan_excl per chunk, a running base
//
// fp64 except where the reference computes in float (the stereo edge's invz, the classification's chi2 and thresholds, 1 / sigma2).  The library is
// compiled with -ffp-contract=off: no product is fused into a sum.  No floating-point atomics: a call's result is the same bits on every run.  Every
// loop has a compile-time bound, so the kernel ends whatever the inputs hold.
#include "hs_poseopt.h"
#include "hs_match_device.h"
#include <cfloat>

#define PO_WAVES (HS_POSE_THREADS / 64)
#define PO_NACC 28                         // 21 of H (upper, row-major), 6 of b, chi
static_assert(sizeof(hs_pose_edge) == 32 && sizeof(hs_pose_problem) == 84 && sizeof(hs_pose_result) == 216, "include/hyslam_amd.h states these layouts");

namespace {

struct PoPose { double w, x, y, z, t[3]; };                       // g2o::SE3Quat: _r (Eigen::Quaterniond) and _t
struct PoCam { double fx, fy, cx, cy, bf; };
typedef float po_f32x4 __attribute__((ext_vector_type(4)));
struct PoEdge { double X[3], u, v, ur, w; bool stereo; };

__device__ __forceinline__ bool po_finite(double x) { return fabs(x) <= DBL_MAX; }                    // g2o_isfinite

// Eigen::Quaterniond(Matrix3d), restated (D13)
__device__ __forceinline__ void po_quat_of(const double m[3][3], PoPose& q)
{
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q.w = 0.5 * t;
        t = 0.5 / t;
        q.x = (m[2][1] - m[1][2]) * t; q.y = (m[0][2] - m[2][0]) * t; q.z = (m[1][0] - m[0][1]) * t;
        return;
    }
    // i = the largest diagonal entry, (i, j, k) cyclic; written out so that no array is indexed by a variable
    const bool i1 = m[1][1] > m[0][0];
    const bool i2 = m[2][2] > (i1 ? m[1][1] : m[0][0]);
    if (i2) {                                                     // i = 2, j = 0, k = 1
        t = sqrt(m[2][2] - m[0][0] - m[1][1] + 1.0);
        q.z = 0.5 * t; t = 0.5 / t;
        q.w = (m[1][0] - m[0][1]) * t; q.x = (m[0][2] + m[2][0]) * t; q.y = (m[1][2] + m[2][1]) * t;
    } else if (i1) {                                              // i = 1, j = 2, k = 0
        t = sqrt(m[1][1] - m[2][2] - m[0][0] + 1.0);
        q.y = 0.5 * t; t = 0.5 / t;
        q.w = (m[0][2] - m[2][0]) * t; q.z = (m[2][1] + m[1][2]) * t; q.x = (m[0][1] + m[1][0]) * t;
    } else {                                                      // i = 0, j = 1, k = 2
        t = sqrt(m[0][0] - m[1][1] - m[2][2] + 1.0);
        q.x = 0.5 * t; t = 0.5 / t;
        q.w = (m[2][1] - m[1][2]) * t; q.y = (m[1][0] + m[0][1]) * t; q.z = (m[2][0] + m[0][2]) * t;
    }
}

// SE3Quat::normalizeRotation(): w >= 0, then Quaterniond::normalize()
__device__ __forceinline__ void po_normalize(PoPose& q)
{
    if (q.w < 0) { q.x = -q.x; q.y = -q.y; q.z = -q.z; q.w = -q.w; }
    const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    q.w = q.w / n; q.x = q.x / n; q.y = q.y / n; q.z = q.z / n;
}

// Quaterniond * Vector3d: v + w * uv + q.vec x uv with uv = 2 (q.vec x v)
__device__ __forceinline__ void po_rotate(const PoPose& q, const double v[3], double out[3])
{
    double ux = q.y * v[2] - q.z * v[1], uy = q.z * v[0] - q.x * v[2], uz = q.x * v[1] - q.y * v[0];
    ux = ux + ux; uy = uy + uy; uz = uz + uz;
    out[0] = v[0] + q.w * ux + (q.y * uz - q.z * uy);
    out[1] = v[1] + q.w * uy + (q.z * ux - q.x * uz);
    out[2] = v[2] + q.w * uz + (q.x * uy - q.y * ux);
}

// SE3Quat::operator*: _t += _r * b._t; _r *= b._r; normalizeRotation()
__device__ __forceinline__ PoPose po_mul(const PoPose& a, const PoPose& b)
{
    PoPose r;
    double rt[3];
    po_rotate(a, b.t, rt);
    r.t[0] = a.t[0] + rt[0]; r.t[1] = a.t[1] + rt[1]; r.t[2] = a.t[2] + rt[2];
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    po_normalize(r);
    return r;
}

// SE3Quat::exp(update): omega = u[0..2], upsilon = u[3..5] (se3quat.h:218-257)
__device__ __forceinline__ PoPose po_exp(const double u[6])
{
    const double theta = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    const double Om[3][3] = {{0.0, -u[2], u[1]}, {u[2], 0.0, -u[0]}, {-u[1], u[0], 0.0}};
    double Om2[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Om2[i][j] = (Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j]) + Om[i][2] * Om[2][j];
    double a, b, c, d;
    if (theta < 0.00001) { a = 1.0; b = 0.5; c = 0.5; d = 1.0 / 6.0; }
    else {
        const double sn = sin(theta), cs = cos(theta);
        a = sn / theta;
        b = (1.0 - cs) / (theta * theta);
        c = b;
        d = (theta - sn) / (theta * theta * theta);
    }
    double R[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double e = i == j ? 1.0 : 0.0;
            R[i][j] = (e + a * Om[i][j]) + b * Om2[i][j];
            V[i][j] = (e + c * Om[i][j]) + d * Om2[i][j];
        }
    PoPose r;
    po_quat_of(R, r);
#pragma unroll
    for (int i = 0; i < 3; i++) r.t[i] = (V[i][0] * u[3] + V[i][1] * u[4]) + V[i][2] * u[5];
    po_normalize(r);
    return r;
}

// Converter::toSE3Quat: the float pose widened, SE3Quat(R, t)
__device__ __forceinline__ PoPose po_from_pose(const float* T)
{
    double m[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) m[i][j] = (double)T[4 * i + j];
    PoPose r;
    po_quat_of(m, r);
    r.t[0] = (double)T[3]; r.t[1] = (double)T[7]; r.t[2] = (double)T[11];
    po_normalize(r);
    return r;
}

// to_homogeneous_matrix(), row-major; the rotation is Quaterniond::toRotationMatrix()
__device__ __forceinline__ void po_matrix(const PoPose& q, double* M)
{
    const double tx = 2.0 * q.x, ty = 2.0 * q.y, tz = 2.0 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w, txx = tx * q.x, txy = ty * q.x, txz = tz * q.x, tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    M[0] = 1.0 - (tyy + tzz); M[1] = txy - twz; M[2] = txz + twy; M[3] = q.t[0];
    M[4] = txy + twz; M[5] = 1.0 - (txx + tzz); M[6] = tyz - twx; M[7] = q.t[1];
    M[8] = txz - twy; M[9] = tyz + twx; M[10] = 1.0 - (txx + tyy); M[11] = q.t[2];
    M[12] = 0.0; M[13] = 0.0; M[14] = 0.0; M[15] = 1.0;
}

__device__ __forceinline__ PoEdge po_load(const hs_pose_edge* e)
{
    const po_f32x4 a = hs_gload<po_f32x4>(e), b = hs_gload<po_f32x4>(reinterpret_cast<const uint8_t*>(e) + 16);
    PoEdge E;
    E.X[0] = (double)a.x; E.X[1] = (double)a.y; E.X[2] = (double)a.z;
    E.u = (double)a.w; E.v = (double)b.x; E.ur = (double)b.y; E.w = (double)b.z;
    E.stereo = !(b.y < 0.0f);                                     // if(views.uR(i)<0) mono, else stereo
    return E;
}

// computeError() and chi2(): p = estimate.map(Xw), e = obs - cam_project(p), chi2 = e . (information * e)
__device__ __forceinline__ double po_error(const PoPose& T, const PoCam& K, const PoEdge& E, double p[3], double e[3])
{
    po_rotate(T, E.X, p);
    p[0] = p[0] + T.t[0]; p[1] = p[1] + T.t[1]; p[2] = p[2] + T.t[2];
    if (E.stereo) {
        const double invz = (double)(float)(1.0 / p[2]);          // const float invz = 1.0f / trans_xyz[2]: a double quotient narrowed to float
        const double r0 = p[0] * invz * K.fx + K.cx;
        e[0] = E.u - r0;
        e[1] = E.v - (p[1] * invz * K.fy + K.cy);
        e[2] = E.ur - (r0 - K.bf * invz);
        return e[0] * (E.w * e[0]) + e[1] * (E.w * e[1]) + e[2] * (E.w * e[2]);
    }
    e[0] = E.u - ((p[0] / p[2]) * K.fx + K.cx);                   // project2d
    e[1] = E.v - ((p[1] / p[2]) * K.fy + K.cy);
    e[2] = 0.0;
    return e[0] * (E.w * e[0]) + e[1] * (E.w * e[1]);
}

// RobustKernelHuber::robustify: rho[0], rho[1]
__device__ __forceinline__ void po_huber(double e, double delta, double& r0, double& r1)
{
    const double dsqr = delta * delta;
    if (e <= dsqr) { r0 = e; r1 = 1.0; return; }
    const double sq = sqrt(e);
    r0 = 2 * sq * delta - dsqr;
    r1 = delta / sq;
}

// the sum of v[i] over the workgroup, the same bits in every thread: xor butterfly over the wave (both partners add the same two numbers), then the
// waves' sums from LDS in wave order
template <int N> __device__ __forceinline__ void po_block_sum(double (&v)[N], double* s_red /*[PO_WAVES * N]*/)
{
#pragma unroll
    for (int i = 0; i < N; i++) {
        double x = v[i];
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) x = x + __shfl_xor(x, s, 64);
        v[i] = x;
    }
    __syncthreads();                                              // the readers of the last sum are done with s_red
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < N; i++) s_red[(threadIdx.x >> 6) * N + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; i++) {
        double x = s_red[i];
#pragma unroll
        for (int w = 1; w < PO_WAVES; w++) x = x + s_red[w * N + i];
        v[i] = x;
    }
}

// (H + lambda I) x = b by LDL^T without pivoting; false where a pivot is not positive (`_cholesky.info() != Eigen::Success`, D13).  H: upper, row-major
__device__ __forceinline__ bool po_ldlt(const double* H, double lambda, const double* b, double* x)
{
    double A[6][6], Lm[6][6], d[6];
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++, k++) { A[i][j] = H[k]; A[j][i] = H[k]; }
#pragma unroll
    for (int i = 0; i < 6; i++) A[i][i] = A[i][i] + lambda;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double s = A[j][j];
#pragma unroll
        for (int c = 0; c < j; c++) s = s - (Lm[j][c] * Lm[j][c]) * d[c];
        if (s <= 0.0) ok = false;
        d[j] = s;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double t = A[i][j];
#pragma unroll
            for (int c = 0; c < j; c++) t = t - (Lm[i][c] * Lm[j][c]) * d[c];
            Lm[i][j] = t / d[j];
        }
    }
    if (!ok) return false;
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = b[i];
#pragma unroll
        for (int c = 0; c < i; c++) s = s - Lm[i][c] * y[c];
        y[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) y[i] = y[i] / d[i];
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int c = i + 1; c < 6; c++) s = s - Lm[c][i] * x[c];
        x[i] = s;
    }
    return true;
}

}  // namespace

__global__ __launch_bounds__(HS_POSE_THREADS) void k_pose_optimize(int Q, const hs_pose_problem* problems, const int64_t* offsets, const int32_t* d_n_edges,
                                                                   int edge_cap, const hs_pose_edge* edges, uint8_t* outlier, hs_pose_result* results)
{
    __shared__ double s_red[PO_WAVES * PO_NACC];
    const int q = blockIdx.x, tid = threadIdx.x;
    if (q >= Q) return;
    int64_t first = 0, n64;
    if (offsets) { first = offsets[q]; n64 = offsets[q + 1] - first; }
    else n64 = min(max((int)*d_n_edges, 0), max(edge_cap, 0));
    const int n = (int)min(max(n64, (int64_t)0), (int64_t)0x7FFFFFFF);
    const hs_pose_edge* E = edges + first;
    uint8_t* flag = outlier + first;
    const hs_pose_problem P = problems[q];
    hs_pose_result* res = results + q;

    if (n < 3) {                                                  // if(nInitialCorrespondences<3) return 0; — pose and flags stay as they are
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 16; i++) { res->Tcw_d[i] = (double)P.Tcw[i]; res->Tcw[i] = P.Tcw[i]; }
            res->n_edges = n; res->n_good = 0; res->rounds = 0; res->lm_iterations = 0; res->lm_trials = 0; res->status = HS_POSE_TOO_FEW;
        }
        return;
    }

    const PoCam K = {(double)P.fx, (double)P.fy, (double)P.cx, (double)P.cy, (double)P.bf};
    const double delta_mono = (double)(float)sqrt(5.991), delta_stereo = (double)(float)sqrt(7.815);   // const float deltaMono = sqrt(5.991)
    const float th_mono = 5.991f, th_stereo = 7.815f;
    const PoPose Tin = po_from_pose(P.Tcw);
    for (int i = tid; i < n; i += HS_POSE_THREADS) flag[i] = 0;   // pFrame->setOutlier(i, false)

    PoPose T = Tin, Terr = Tin;                                   // the estimate; the estimate the edges' errors belong to (D14)
    bool robust = true;
    int n_bad = 0, rounds = 0, iterations = 0, trials = 0;
    for (int rnd = 0; rnd < 4; rnd++) {
        T = Tin; Terr = Tin;                                      // vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw))
        if (n - n_bad > 0) {                                      // no active edge: optimize() returns -1 and nothing moves
            double lambda = 0.0, ni = 2.0;
            double dx[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int it = 0; it < 10; it++) {
                // computeActiveErrors(); activeRobustChi2(); buildSystem()
                double acc[PO_NACC];
#pragma unroll
                for (int i = 0; i < PO_NACC; i++) acc[i] = 0.0;
                for (int i = tid; i < n; i += HS_POSE_THREADS) {
                    if (flag[i]) continue;
                    const PoEdge e = po_load(E + i);
                    double p[3], er[3];
                    const double chi = po_error(T, K, e, p, er);
                    double r0 = chi, r1 = 1.0;
                    if (robust) po_huber(chi, e.stereo ? delta_stereo : delta_mono, r0, r1);
                    acc[27] = acc[27] + r0;
                    const double x = p[0], y = p[1], invz = 1.0 / p[2], invz_2 = invz * invz;
                    double J[3][6];
                    J[0][0] = x * y * invz_2 * K.fx; J[0][1] = -(1 + (x * x * invz_2)) * K.fx; J[0][2] = y * invz * K.fx;
                    J[0][3] = -invz * K.fx; J[0][4] = 0.0; J[0][5] = x * invz_2 * K.fx;
                    J[1][0] = (1 + y * y * invz_2) * K.fy; J[1][1] = -x * y * invz_2 * K.fy; J[1][2] = -x * invz * K.fy;
                    J[1][3] = 0.0; J[1][4] = -invz * K.fy; J[1][5] = y * invz_2 * K.fy;
                    J[2][0] = J[0][0] - K.bf * y * invz_2; J[2][1] = J[0][1] + K.bf * x * invz_2; J[2][2] = J[0][2];
                    J[2][3] = J[0][3]; J[2][4] = 0.0; J[2][5] = J[0][5] - K.bf * invz_2;
                    // b -= rho[1] * A^T * omega * e;  H += A^T * (rho[1] * omega) * A;  without a kernel there is no rho[1] (base_unary_edge.hpp:62-73)
                    const double ww = robust ? r1 * e.w : e.w;
                    int k = 0;
#pragma unroll
                    for (int a = 0; a < 6; a++) {
                        double s = robust ? ((r1 * J[0][a]) * e.w) * er[0] + ((r1 * J[1][a]) * e.w) * er[1] : (J[0][a] * e.w) * er[0] + (J[1][a] * e.w) * er[1];
                        if (e.stereo) s = s + (robust ? ((r1 * J[2][a]) * e.w) * er[2] : (J[2][a] * e.w) * er[2]);
                        acc[21 + a] = acc[21 + a] - s;
#pragma unroll
                        for (int c = a; c < 6; c++, k++) {
                            double h = (J[0][a] * ww) * J[0][c] + (J[1][a] * ww) * J[1][c];
                            if (e.stereo) h = h + (J[2][a] * ww) * J[2][c];
                            acc[k] = acc[k] + h;
                        }
                    }
                }
                po_block_sum<PO_NACC>(acc, s_red);
                Terr = T;
                iterations++;
                const double* H = acc;
                const double* b = acc + 21;
                double current = acc[27];
                if (it == 0) {                                    // computeLambdaInit(): tau * max |H_jj|
                    double maxd = 0.0;
                    int k = 0;
#pragma unroll
                    for (int j = 0; j < 6; j++) { const double a = fabs(H[k]); maxd = a < maxd ? maxd : a; k += 6 - j; }
                    lambda = 1e-5 * maxd;
                    ni = 2.0;
                }
                double rho = 0.0;
                int qmax = 0;
                for (int trial = 0; trial < 10; trial++) {        // do { ... } while (rho < 0 && qmax < 10)
                    trials++;
                    double x[6];
                    const bool ok2 = po_ldlt(H, lambda, b, x);    // a failed factorisation leaves the last solution in x (zero before the first)
                    if (ok2) {
#pragma unroll
                        for (int j = 0; j < 6; j++) dx[j] = x[j];
                    }
                    const PoPose backup = T;                      // push()
                    T = po_mul(po_exp(dx), T);                    // oplusImpl: setEstimate(SE3Quat::exp(update) * estimate())
                    double chi[1] = {0.0};
                    for (int i = tid; i < n; i += HS_POSE_THREADS) {
                        if (flag[i]) continue;
                        const PoEdge e = po_load(E + i);
                        double p[3], er[3];
                        const double c = po_error(T, K, e, p, er);
                        double r0 = c, r1 = 1.0;
                        if (robust) po_huber(c, e.stereo ? delta_stereo : delta_mono, r0, r1);
                        chi[0] = chi[0] + r0;
                    }
                    po_block_sum<1>(chi, s_red);
                    Terr = T;
                    double temp = chi[0];
                    if (!ok2) temp = DBL_MAX;
                    double scale = 0.0;                           // computeScale()
#pragma unroll
                    for (int j = 0; j < 6; j++) scale = scale + dx[j] * (lambda * dx[j] + b[j]);
                    scale = scale + 1e-3;
                    rho = (current - temp) / scale;
                    if (rho > 0 && po_finite(temp)) {
                        const double t = 2 * rho - 1;
                        double alpha = 1. - t * t * t;
                        alpha = (2. / 3.) < alpha ? (2. / 3.) : alpha;
                        lambda = lambda * ((1. / 3.) < alpha ? alpha : (1. / 3.));
                        ni = 2.0;
                        current = temp;
                    } else {
                        lambda = lambda * ni;
                        ni = ni * 2;
                        T = backup;                               // pop()
                        if (!po_finite(lambda)) break;
                    }
                    qmax++;
                    if (!(rho < 0 && qmax < 10)) break;
                }
                if (qmax == 10 || rho == 0 || !po_finite(lambda)) break;   // Terminate
            }
        }
        // classification (Optimizer.cc:209-266): an outlier gets computeError() at the estimate, an inlier keeps the error of the last
        // computeActiveErrors(), which after a rejected trial is the rejected estimate's
        double bad[1] = {0.0};
        for (int i = tid; i < n; i += HS_POSE_THREADS) {
            const PoEdge e = po_load(E + i);
            double p[3], er[3];
            const float chi2 = (float)(flag[i] ? po_error(T, K, e, p, er) : po_error(Terr, K, e, p, er));   // const float chi2 = e->chi2();
            const uint8_t f = chi2 > (e.stereo ? th_stereo : th_mono) ? 1 : 0;                             // false for NaN: an inlier
            flag[i] = f;
            bad[0] = bad[0] + (double)f;
        }
        po_block_sum<1>(bad, s_red);
        n_bad = (int)bad[0];
        rounds++;
        if (rnd == 2) robust = false;                             // e->setRobustKernel(0)
        if (n < 10) break;                                        // if(optimizer.edges().size()<10) break;
    }

    if (tid == 0) {
        double M[16];
        po_matrix(T, M);
        bool finite = true;
#pragma unroll
        for (int i = 0; i < 16; i++) { res->Tcw_d[i] = M[i]; res->Tcw[i] = (float)M[i]; finite = finite && po_finite(M[i]); }
        res->n_edges = n; res->n_good = n - n_bad; res->rounds = rounds; res->lm_iterations = iterations; res->lm_trials = trials;
        res->status = finite ? HS_POSE_OK : HS_POSE_NONFINITE;
    }
}

__global__ __launch_bounds__(1024) void k_pose_edges(hs_frame_view F, const hs_landmark* lms, int L, const int32_t* kp_lm, float sigma_ref, hs_pose_edge* out,
                                                     int cap, int32_t* n_edges)
{
    __shared__ uint32_t s_wave[16];
    const int tid = threadIdx.x;
    uint32_t base = 0;
    for (int i0 = 0; i0 < F.n; i0 += 1024) {
        const int i = i0 + tid;
        const int lm = i < F.n ? kp_lm[i] : -1;
        const uint32_t keep = (unsigned)lm < (unsigned)L ? 1u : 0u;                       // MapPoint* pMP = pFrame->hasAssociation(i); if(pMP)
        uint32_t total;
        const uint32_t pos = base + block_scan_excl(keep, s_wave, total);
        if (keep && pos < (uint32_t)max(cap, 0)) {
            const hs_keypoint kp = F.kps[i];
            const float s = __fdiv_rn(kp.size, F.size_ref);                                // determineSigma2 (FeatureExtractorSettings.cpp:5-8), in float
            hs_pose_edge e;
            e.Xw[0] = lms[lm].pos[0]; e.Xw[1] = lms[lm].pos[1]; e.Xw[2] = lms[lm].pos[2];
            e.u = kp.x; e.v = kp.y; e.ur = F.uR ? F.uR[i] : -1.0f;
            e.inv_sigma2 = __fdiv_rn(1.0f, __fmul_rn(sigma_ref, __fmul_rn(s, s)));          // const float invSigma2 = 1/orb_params.determineSigma2(kpUn.size)
            e.kp = i;
            out[pos] = e;
        }
        base += total;
        __syncthreads();                                                                   // s_wave is rewritten by the next chunk
    }
    if (tid == 0) *n_edges = (int32_t)base;
}

void hs_launch_pose_optimize(int Q, const hs_pose_problem* d_problems, const int64_t* d_edge_offsets, const int32_t* d_n_edges, int edge_cap,
                             const hs_pose_edge* d_edges, uint8_t* d_outlier, hs_pose_result* d_results, hipStream_t s)
{
    if (Q <= 0) return;
    hipLaunchKernelGGL(k_pose_optimize, dim3(Q), dim3(HS_POSE_THREADS), 0, s, Q, d_problems, d_edge_offsets, d_n_edges, edge_cap, d_edges, d_outlier, d_results);
}

void hs_launch_pose_edges(const hs_frame_view& F, const hs_landmark* d_lms, int L, const int32_t* d_kp_lm, float sigma_ref, hs_pose_edge* d_edges, int cap,
                          int32_t* d_n_edges, hipStream_t s)
{
    hipLaunchKernelGGL(k_pose_edges, dim3(1), dim3(1024), 0, s, F, d_lms, L, d_kp_lm, sigma_ref, d_edges, cap, d_n_edges);
}
