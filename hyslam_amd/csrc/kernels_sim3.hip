// kernels_sim3.hip — batched Horn Sim3 RANSAC (Sim3Solver, src/estimators/Sim3Solver.cc).
//   k_sim3_hypotheses  grid (ceil(H / 64), problems), one LANE per hypothesis: the sample of absolute iteration `it` (three draws that write the back
//                      element to the place named by the drawn VALUE), ComputeSim3 on its three points, then CheckInliers over all N: the workgroup
//                      stages the correspondences in LDS in chunks of HS_SIM3_CHUNK records (the two points, their own projections, the two
//                      thresholds) and every lane walks the chunk with its own T12 and T21; writes the count and R, t, s
//   k_sim3_select      one wave per problem: walks the counts in order (the reference's acceptance), recomputes the mask of the chosen hypothesis
//                      from its stored pose — the same instructions on the same inputs as the count — and writes the state, the result, the masks
// A hypothesis is a 3-point closed form and a 4x4 Jacobi: no parallelism inside, so a lane owns it from the sample to the count.  Nothing is reduced
// across lanes, there is no atomic and no floating-point sum shared between lanes: there is no summation order to state.  All lanes of a wave read the
// same LDS word at the same time (a broadcast).  -ffp-contract=off; divide and sqrt correctly rounded; every loop has a bound that no input
// extends (HS_SIM3_EIG_SWEEPS sweeps, ceil(N / HS_SIM3_CHUNK) chunks, `passes` counts).  The math is __host__ __device__, so a host build of this
// file computes the same bits (tests/cpp/sim3_sanitize/sim3_host_math.cpp).
#include "hs_sim3.h"
#include <algorithm>
#include <cmath>

static_assert(sizeof(hs_sim3_corr) == 48 && sizeof(hs_sim3_params) == 64 && sizeof(hs_sim3_state) == 128 && sizeof(hs_sim3_result) == 136 && sizeof(hs_sim3_plan_t) == 8,
              "include/hyslam_amd.h states these layouts");

#define SIM3_HD __host__ __device__
#define SIM3_REC 12                      // floats of a staged record: X1c[3], X2c[3], P1im1[2], P2im2[2], the two thresholds

namespace {

struct Sim3Pose { float R[9], t[3], s; };
struct Sim3Xf { float a[12], b[12]; };   // the upper three rows of T12 = [sR | t] and of T21 = [(1/s)Rt | -(1/s)Rt t]

// mvnMaxError (:91-92, Sim3Solver.h:77-78): the double 9.210 * sigma2 stored in a size_t, compared as a float (:360).  Where the conversion is
// undefined (NaN, negative, 2^64 and above) the threshold is 0.
SIM3_HD float sim3_threshold(float sigma2)
{
    const double d = 9.210 * (double)sigma2;
    if (!(d >= 0.0) || d >= 18446744073709551616.0) return 0.f;
    return (float)(unsigned long long)d;
}
// FromCameraToImage (:409-427)
SIM3_HD void sim3_image(const float* X, const float* k, float* uv)
{
    const float invz = 1 / X[2];
    const float x = X[0] * invz, y = X[1] * invz;
    uv[0] = k[0] * x + k[2]; uv[1] = k[1] * y + k[3];
}
SIM3_HD void sim3_record(const hs_sim3_corr& c, const float* k1, const float* k2, float* r)
{
    r[0] = c.X1c[0]; r[1] = c.X1c[1]; r[2] = c.X1c[2]; r[3] = c.X2c[0]; r[4] = c.X2c[1]; r[5] = c.X2c[2];
    sim3_image(c.X1c, k1, r + 6);
    sim3_image(c.X2c, k2, r + 8);
    r[10] = sim3_threshold(c.sigma2_1); r[11] = sim3_threshold(c.sigma2_2);
}
// Project (:386-407): Rcw * X + tcw is one fused product (D19: double accumulation in index order, one narrowing), the rest float
SIM3_HD void sim3_project(const float* T, const float* X, const float* k, float* uv)
{
    float P[3];
    for (int i = 0; i < 3; i++)
        P[i] = (float)((((double)T[4 * i] * (double)X[0] + (double)T[4 * i + 1] * (double)X[1]) + (double)T[4 * i + 2] * (double)X[2]) + (double)T[4 * i + 3]);
    sim3_image(P, k, uv);
}
// CheckInliers (:344-368) for one record; a NaN fails a strict <
SIM3_HD bool sim3_inlier(const Sim3Xf& xf, const float* k1, const float* k2, const float* r)
{
    float q[2];
    sim3_project(xf.a, r + 3, k1, q);                              // 2 into 1
    const float a0 = r[6] - q[0], a1 = r[7] - q[1];
    const float err1 = (float)((double)a0 * (double)a0 + (double)a1 * (double)a1);
    sim3_project(xf.b, r, k2, q);                                  // 1 into 2
    const float b0 = q[0] - r[8], b1 = q[1] - r[9];
    const float err2 = (float)((double)b0 * (double)b0 + (double)b1 * (double)b1);
    return err1 < r[10] && err2 < r[11];
}

// one rotation of the cyclic Jacobi (D19) on the symmetric A, V <- V J; an exactly zero (or NaN) off-diagonal entry is skipped
SIM3_HD void sim3_rotate(double (*A)[4], double (*V)[4], int p, int q)
{
    const double apq = A[p][q];
    if (!(fabs(apq) > 0.0)) return;
    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    for (int k = 0; k < 4; k++) {
        const double x = A[k][p], y = A[k][q];
        A[k][p] = c * x - s * y; A[k][q] = s * x + c * y;
    }
    for (int k = 0; k < 4; k++) {
        const double x = A[p][k], y = A[q][k];
        A[p][k] = c * x - s * y; A[q][k] = s * x + c * y;
    }
    for (int k = 0; k < 4; k++) {
        const double x = V[k][p], y = V[k][q];
        V[k][p] = c * x - s * y; V[k][q] = s * x + c * y;
    }
}

// ComputeSim3 (:230-341) on three correspondences, x[k][r] = coordinate r of point k; D19 defines what OpenCV does inside
SIM3_HD void sim3_solve(const float (*x1)[3], const float (*x2)[3], int fix_scale, Sim3Pose* o)
{
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3], M[3][3];            // Pr[r][k]: row r, column (point) k
    for (int r = 0; r < 3; r++) {
        O1[r] = ((x1[0][r] + x1[1][r]) + x1[2][r]) / 3.0f;
        O2[r] = ((x2[0][r] + x2[1][r]) + x2[2][r]) / 3.0f;
        for (int k = 0; k < 3; k++) { Pr1[r][k] = x1[k][r] - O1[r]; Pr2[r][k] = x2[k][r] - O2[r]; }
    }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            M[i][j] = (float)(((double)Pr2[i][0] * (double)Pr1[j][0] + (double)Pr2[i][1] * (double)Pr1[j][1]) + (double)Pr2[i][2] * (double)Pr1[j][2]);
    const double m00 = M[0][0], m01 = M[0][1], m02 = M[0][2], m10 = M[1][0], m11 = M[1][1], m12 = M[1][2], m20 = M[2][0], m21 = M[2][1], m22 = M[2][2];
    const float N11 = (float)(m00 + m11 + m22), N12 = (float)(m12 - m21), N13 = (float)(m20 - m02), N14 = (float)(m01 - m10);
    const float N22 = (float)(m00 - m11 - m22), N23 = (float)(m01 + m10), N24 = (float)(m20 + m02);
    const float N33 = (float)(-m00 + m11 - m22), N34 = (float)(m12 + m21), N44 = (float)(-m00 - m11 + m22);
    double A[4][4] = { { N11, N12, N13, N14 }, { N12, N22, N23, N24 }, { N13, N23, N33, N34 }, { N14, N24, N34, N44 } };
    double V[4][4] = { { 1, 0, 0, 0 }, { 0, 1, 0, 0 }, { 0, 0, 1, 0 }, { 0, 0, 0, 1 } };
    for (int sweep = 0; sweep < HS_SIM3_EIG_SWEEPS; sweep++) {
        sim3_rotate(A, V, 0, 1); sim3_rotate(A, V, 0, 2); sim3_rotate(A, V, 0, 3);
        sim3_rotate(A, V, 1, 2); sim3_rotate(A, V, 1, 3); sim3_rotate(A, V, 2, 3);
    }
    double lam = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
    for (int j = 1; j < 4; j++)                                    // the first of equal eigenvalues
        if (A[j][j] > lam) { lam = A[j][j]; w = V[0][j]; x = V[1][j]; y = V[2][j]; z = V[3][j]; }
    if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
    // R from the quaternion, homogeneous form: the matrix cv::Rodrigues gives for the angle-axis 2 atan2(|v|, w) v / |v|
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    const double n = ((ww + xx) + yy) + zz;
    double R[9] = { (((ww + xx) - yy) - zz) / n, (2.0 * (xy - wz)) / n, (2.0 * (xz + wy)) / n,
                    (2.0 * (xy + wz)) / n, (((ww - xx) + yy) - zz) / n, (2.0 * (yz - wx)) / n,
                    (2.0 * (xz - wy)) / n, (2.0 * (yz + wx)) / n, (((ww - xx) - yy) + zz) / n };
    if (x == 0.0 && y == 0.0 && z == 0.0) {                        // :284 divides 0 by 0: kept
        const double nan = (x * 0.0) / (y * 0.0);
        for (int i = 0; i < 9; i++) R[i] = nan;
    }
    for (int i = 0; i < 9; i++) o->R[i] = (float)R[i];
    if (fix_scale) o->s = 1.0f;
    else {
        double nom = 0.0, den = 0.0;
        for (int i = 0; i < 3; i++)
            for (int k = 0; k < 3; k++) {
                const float p3 = (float)(((double)o->R[3 * i] * (double)Pr2[0][k] + (double)o->R[3 * i + 1] * (double)Pr2[1][k]) + (double)o->R[3 * i + 2] * (double)Pr2[2][k]);
                nom = nom + (double)Pr1[i][k] * (double)p3;
                den = den + (double)(p3 * p3);
            }
        o->s = (float)(nom / den);
    }
    for (int i = 0; i < 3; i++)
        o->t[i] = (float)((double)O1[i] - (double)o->s * (((double)o->R[3 * i] * (double)O2[0] + (double)o->R[3 * i + 1] * (double)O2[1]) + (double)o->R[3 * i + 2] * (double)O2[2]));
}

// steps 8.1 and 8.2 (:322-340)
SIM3_HD void sim3_transforms(const Sim3Pose& o, Sim3Xf* xf)
{
    const double alpha = 1.0 / (double)o.s;
    float inv[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { xf->a[4 * i + j] = o.s * o.R[3 * i + j]; inv[i][j] = (float)(alpha * (double)o.R[3 * j + i]); }
    for (int i = 0; i < 3; i++) {
        xf->a[4 * i + 3] = o.t[i];
        for (int j = 0; j < 3; j++) xf->b[4 * i + j] = inv[i][j];
        xf->b[4 * i + 3] = (float)(-(((double)inv[i][0] * (double)o.t[0] + (double)inv[i][1] * (double)o.t[1]) + (double)inv[i][2] * (double)o.t[2]));
    }
}

// the sample of absolute iteration `it` (:167-181): three draws that write the back element to the place named by the drawn VALUE (hs_ransac.h)
SIM3_HD void sim3_sample(const HsSim3Problem& p, long long it, const uint32_t* draws, int draw_cap, int* sample)
{
    hs_ransac_sample<3, /*WRITE_AT_VALUE=*/true>(p, 3, draws, draw_cap, HS_SIM3_DRAW_STRIDE, it, sample);
}
// the acceptance (:187-204) over the counts c[0 .. m) of hypotheses base .. base+m-1: returns the index that returns out of the loop, or -1
SIM3_HD int sim3_walk(const int* c, int m, int base, int min_inliers, int* best, int* rec)
{
    for (int k = 0; k < m; k++)
        if (c[k] >= *best) {
            *best = c[k]; *rec = base + k;
            if (c[k] > min_inliers) return base + k;
        }
    return -1;
}
SIM3_HD bool sim3_finite(const Sim3Pose& o, const Sim3Xf& xf)
{
    bool f = o.s - o.s == 0.f;                                     // v - v is 0 for a finite v and a NaN otherwise
    for (int i = 0; i < 9; i++) f = f && o.R[i] - o.R[i] == 0.f;
    for (int i = 0; i < 3; i++) f = f && o.t[i] - o.t[i] == 0.f;
    for (int i = 0; i < 12; i++) f = f && xf.a[i] - xf.a[i] == 0.f;
    return f;
}

#ifndef HS_SIM3_MATH_ONLY               // a host program that times or checks the math alone (tests/cpp/bench_sim3_host.cpp) stops here
__global__ __launch_bounds__(64) void k_sim3_hypotheses(const HsSim3Batch B, const hs_sim3_corr* __restrict__ corrs, int n_iterations, const uint32_t* __restrict__ draws,
                                                        int draw_cap, const hs_sim3_state* __restrict__ states, int H, int32_t* __restrict__ hyp_count,
                                                        float* __restrict__ hyp_pose)
{
    __shared__ float s_rec[HS_SIM3_CHUNK * SIM3_REC];
    const HsSim3Problem& p = B.p[blockIdx.y];
    if (p.n < p.min_inliers || p.n < 3) return;
    const int it0 = hs_ransac_it0(states[p.q].iterations);
    const int passes = hs_ransac_passes_and(it0, p.max_its, n_iterations, H);
    if ((int)(blockIdx.x * 64) >= passes) return;                 // the whole workgroup
    const int lane = threadIdx.x;
    const int j = (int)(blockIdx.x * 64) + lane;
    const bool active = j < passes;
    const hs_sim3_corr* pc = corrs + p.off;
    Sim3Pose pose;
    Sim3Xf xf;
    if (active) {
        int s[3];
        float x1[3][3], x2[3][3];
        sim3_sample(p, (long long)it0 + j, draws, draw_cap, s);
        for (int k = 0; k < 3; k++)
            for (int r = 0; r < 3; r++) { x1[k][r] = pc[s[k]].X1c[r]; x2[k][r] = pc[s[k]].X2c[r]; }
        sim3_solve(x1, x2, p.fix_scale, &pose);
        sim3_transforms(pose, &xf);
    }
    int cnt = 0;
    for (int base = 0; base < p.n; base += HS_SIM3_CHUNK) {       // p.n <= 2^31 - 1 and base <= p.n - 1 before the step: the sum below is formed in 64 bits
        const int m = p.n - base < HS_SIM3_CHUNK ? p.n - base : HS_SIM3_CHUNK;
        __syncthreads();
        for (int i = lane; i < m; i += 64) sim3_record(pc[(size_t)base + (size_t)i], p.k1, p.k2, s_rec + SIM3_REC * i);
        __syncthreads();
        if (active)
            for (int i = 0; i < m; i++) cnt += sim3_inlier(xf, p.k1, p.k2, s_rec + SIM3_REC * i) ? 1 : 0;
        if (p.n - base <= HS_SIM3_CHUNK) break;                   // no `base` past 2^31 - 1
    }
    if (active) {
        const size_t slot = (size_t)p.q * (size_t)H + (size_t)j;
        hyp_count[slot] = cnt;
        float* o = hyp_pose + slot * HS_SIM3_POSE_WORDS;
        for (int i = 0; i < 9; i++) o[i] = pose.R[i];
        for (int i = 0; i < 3; i++) o[9 + i] = pose.t[i];
        o[12] = pose.s; o[13] = 0.f; o[14] = 0.f; o[15] = 0.f;
    }
}

__global__ __launch_bounds__(64) void k_sim3_select(const HsSim3Batch B, const hs_sim3_corr* __restrict__ corrs, int n_iterations, hs_sim3_state* __restrict__ states,
                                                    uint8_t* __restrict__ best_masks, hs_sim3_result* __restrict__ results, uint8_t* __restrict__ inlier_masks, int H,
                                                    const int32_t* __restrict__ hyp_count, const float* __restrict__ hyp_pose)
{
    __shared__ int s_cnt[64];
    const HsSim3Problem& p = B.p[blockIdx.x];
    const int lane = threadIdx.x;
    hs_sim3_state* st = states + p.q;
    hs_sim3_result* res = results + p.q;
    const hs_sim3_corr* pc = corrs + p.off;
    uint8_t* best_mask = best_masks + p.off;
    uint8_t* out_mask = inlier_masks + p.off;
    const int iterations0 = st->iterations;
    int best = hs_ransac_it0(st->best_inliers);                    // a negative count reads as 0, like mnIterations
    __syncthreads();                                              // the state is read before lane 0 writes it
    if (p.n < p.min_inliers || p.n < 3) {                          // :150-154; below three points the reference would sample from an empty list
        for (long long i = lane; i < p.n; i += 64) out_mask[i] = 0;
        if (lane == 0) {
            hs_sim3_result r{};
            r.status = HS_SIM3_TOO_FEW; r.iterations = iterations0;
            *res = r;
        }
        return;
    }
    const int it0 = hs_ransac_it0(iterations0);
    const int passes = hs_ransac_passes_and(it0, p.max_its, n_iterations, H);
    int rec = -1, found = -1;
    for (int base = 0; base < passes && found < 0; base += 64) {
        const int m = passes - base < 64 ? passes - base : 64;
        __syncthreads();
        s_cnt[lane] = lane < m ? hyp_count[(size_t)p.q * (size_t)H + (size_t)base + (size_t)lane] : 0;
        __syncthreads();
        found = sim3_walk(s_cnt, m, base, p.min_inliers, &best, &rec);     // every lane, the same words
    }
    Sim3Pose pose{};
    Sim3Xf xf{};
    if (rec >= 0) {
        const float* o = hyp_pose + ((size_t)p.q * (size_t)H + (size_t)rec) * HS_SIM3_POSE_WORDS;
        for (int i = 0; i < 9; i++) pose.R[i] = o[i];
        for (int i = 0; i < 3; i++) pose.t[i] = o[9 + i];
        pose.s = o[12];
        sim3_transforms(pose, &xf);
        for (long long i = lane; i < p.n; i += 64) {
            float r[SIM3_REC];
            sim3_record(pc[i], p.k1, p.k2, r);
            const uint8_t in = sim3_inlier(xf, p.k1, p.k2, r) ? 1 : 0;
            best_mask[i] = in;
            out_mask[i] = found >= 0 ? in : 0;
        }
    } else
        for (long long i = lane; i < p.n; i += 64) out_mask[i] = 0;
    if (lane == 0) {
        hs_sim3_result r{};
        const int done = found >= 0 ? it0 + found + 1 : it0 + passes;
        if (rec >= 0) {
            hs_sim3_state s{};
            s.iterations = done; s.best_inliers = best; s.s = pose.s;
            for (int i = 0; i < 9; i++) s.R[i] = pose.R[i];
            for (int i = 0; i < 3; i++) s.t[i] = pose.t[i];
            for (int i = 0; i < 12; i++) s.T12[i] = xf.a[i];
            s.T12[15] = 1.f;
            *st = s;
        } else
            st->iterations = done;
        if (found >= 0) {
            for (int i = 0; i < 12; i++) r.T12[i] = xf.a[i];
            r.T12[15] = 1.f;
            for (int i = 0; i < 9; i++) r.R[i] = pose.R[i];
            for (int i = 0; i < 3; i++) r.t[i] = pose.t[i];
            r.s = pose.s;
            r.status = sim3_finite(pose, xf) ? HS_SIM3_FOUND : HS_SIM3_NONFINITE;
            r.n_inliers = best; r.at_iteration = done;
        } else
            r.status = done >= p.max_its ? HS_SIM3_EXHAUSTED : HS_SIM3_CONTINUE;
        r.iterations = done; r.hypotheses_run = passes;
        *res = r;
    }
}
#endif
}  // namespace

#ifndef HS_SIM3_MATH_ONLY
int hs_sim3_call_bound(int Q, const hs_sim3_params* params, const int64_t* corr_offsets, int n_iterations)
{
    int H = 1;
    for (int q = 0; q < Q; q++) {
        hs_sim3_plan_t plan;
        if (hs_sim3_plan((int)(corr_offsets[q + 1] - corr_offsets[q]), &params[q], &plan) == HS_OK)
            H = std::max(H, hs_ransac_passes_and(0, plan.max_iterations, n_iterations, INT_MAX));
    }
    return H;
}

void hs_launch_sim3_iterate(const HsSim3Args& a, void* d_work, hipStream_t s)
{
    const int H = hs_sim3_call_bound(a.Q, a.params, a.corr_offsets, a.n_iterations);
    HsWorkCursor cur(d_work);
    const HsSim3Work w(cur, a.Q, a.corr_offsets[a.Q], H);
    hs_ransac_for_batches(a.Q, HS_SIM3_BATCH, [&](int q0, int nb) {
        HsSim3Batch B{};
        for (int b = 0; b < nb; b++) {
            const int q = q0 + b;
            const hs_sim3_params& pp = a.params[q];
            hs_sim3_plan_t plan;
            HsSim3Problem& o = B.p[b];
            o.off = a.corr_offsets[q]; o.n = (int)(a.corr_offsets[q + 1] - a.corr_offsets[q]); o.seed = pp.seed;
            (void)hs_sim3_plan(o.n, &pp, &plan);
            o.min_inliers = pp.min_inliers; o.max_its = plan.max_iterations; o.fix_scale = pp.fix_scale;
            o.k1[0] = pp.fx1; o.k1[1] = pp.fy1; o.k1[2] = pp.cx1; o.k1[3] = pp.cy1;
            o.k2[0] = pp.fx2; o.k2[1] = pp.fy2; o.k2[2] = pp.cx2; o.k2[3] = pp.cy2;
            o.q = q;
        }
        hipLaunchKernelGGL(k_sim3_hypotheses, dim3(((unsigned)H + 63u) / 64u, (unsigned)nb), dim3(64), 0, s, B, a.corrs, a.n_iterations, a.draws, a.draw_cap, a.states, H,
                           w.hyp_count, w.hyp_pose);
        hipLaunchKernelGGL(k_sim3_select, dim3((unsigned)nb), dim3(64), 0, s, B, a.corrs, a.n_iterations, a.states, a.best_masks, a.results, a.inlier_masks, H, w.hyp_count,
                           w.hyp_pose);
    });
}
#endif
