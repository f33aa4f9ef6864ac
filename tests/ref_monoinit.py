"""Reference for the monocular initialisation (MonoEstimator, src/initializers/MonoEstimator.cpp), twice.

LITERAL      a numpy restatement of the source under D18 (the draws), D20 (the linear algebra) and D21 (the parallax as a cosine): float32 where the
             reference computes in float, one IEEE operation per numpy operation in the order the source writes them, every decomposition the
             one-sided cyclic Jacobi of D17 on widened operands.  Vectorised ACROSS hypotheses (and across the points of a CheckRT), sequential in
             the match index, so every score is the sum the sequential loop forms.  This is what the library must EQUAL.
INDEPENDENT  the same algorithm with numpy.linalg.svd / inv / det on float64 for every piece of linear algebra and math.acos for the parallax,
             which is then compared in DEGREES as the source does.  It shares no decomposition with LITERAL; tests/test_monoinit_ref.py measures how
             far the two are apart.

estimate(kps1, kps2, matches12, params, draws, kind) -> dict: everything hs_monoinit_result holds, the two masks, p3d, triangulated, and per
hypothesis the scores and models (`hyp`).
"""
import math

import numpy as np

import ref_pnp

F32, F64 = np.float32, np.float64
EPS = F64(np.finfo(np.float64).eps)
SVD_SWEEPS = 30
DRAW_STRIDE = 8
TOO_FEW, FAILED, OK_H, OK_F, NONFINITE = 0, 1, 2, 3, 4
MODEL_NONE, MODEL_H, MODEL_F = 0, 1, 2
DEFAULT = dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0, sigma=1.0, max_iterations=200, min_triangulated=50, min_frac_triangulated=0.9, min_parallax_deg=1.0,
               seed=0)


def cos_min_parallax(deg):
    """D21: the float nearest cos(min_parallax_deg * pi / 180)"""
    return F32(math.cos(float(F32(deg)) * 3.14159265358979323846 / 180.0))


# ---------------------------------------------------------------- the draws and the sampler (D18; hs_ransac_sample<8, false>)
def sample_sets(N, max_iterations, seed, draws=None):
    return [ref_pnp.sample(N, 8, [ref_pnp.draw32(seed, it, k, 8, draws) for k in range(8)]) for it in range(max_iterations)]


# ---------------------------------------------------------------- D17's Jacobi, batched: A [B, m, n] -> G = U Sigma, V, sig [B, n], perm [B, n]
def jacobi_batch(A):
    G = np.array(A, F64)
    B, m, n = G.shape
    V = np.zeros((B, n, n), F64)
    V[:, np.arange(n), np.arange(n)] = 1.0
    f2 = np.zeros(B, F64)
    for i in range(m):
        for j in range(n):
            f2 = f2 + G[:, i, j] * G[:, i, j]
    tiny = (F64(n) * EPS) * (F64(n) * EPS) * f2
    with np.errstate(all="ignore"):
        for _ in range(SVD_SWEEPS):
            any_rot = False
            for p in range(n - 1):
                for q in range(p + 1, n):
                    a, b, g = np.zeros(B, F64), np.zeros(B, F64), np.zeros(B, F64)
                    for i in range(m):
                        gp, gq = G[:, i, p], G[:, i, q]
                        a = a + gp * gp
                        b = b + gq * gq
                        g = g + gp * gq
                    rot = (a > tiny) & (b > tiny) & (np.abs(g) > EPS * np.sqrt(a * b))
                    if not rot.any():
                        continue
                    any_rot = True
                    zeta = (b - a) / (F64(2) * g)
                    t = np.where(zeta < 0, F64(-1), F64(1)) / (np.abs(zeta) + np.sqrt(F64(1) + zeta * zeta))
                    c = F64(1) / np.sqrt(F64(1) + t * t)
                    s = c * t
                    for M in (G, V):
                        x, y = M[:, :, p].copy(), M[:, :, q].copy()
                        M[:, :, p] = np.where(rot[:, None], c[:, None] * x - s[:, None] * y, x)
                        M[:, :, q] = np.where(rot[:, None], s[:, None] * x + c[:, None] * y, y)
            if not any_rot:
                break
        sig = np.zeros((B, n), F64)
        for j in range(n):
            s = np.zeros(B, F64)
            for i in range(m):
                s = s + G[:, i, j] * G[:, i, j]
            sig[:, j] = np.sqrt(s)
    perm = np.zeros((B, n), np.int64)
    for j in range(n):                                             # stable, descending: the place pnp_svd's insertion sort gives column j
        rank = np.zeros(B, np.int64)
        for k in range(n):
            if k < j:
                rank += ~(sig[:, k] < sig[:, j])
            elif k > j:
                rank += sig[:, j] < sig[:, k]
        perm[np.arange(B), rank] = j
    return G, V, sig, perm


def _col(M, c):
    """column c[b] of M[b]"""
    return M[np.arange(len(M)), :, c]


# ---------------------------------------------------------------- D19 / D20 on float32 operands, any leading batch shape
def mul33(a, b):
    a, b = np.asarray(a, F32).astype(F64), np.asarray(b, F32).astype(F64)
    o = (a[..., :, 0, None] * b[..., None, 0, :] + a[..., :, 1, None] * b[..., None, 1, :]) + a[..., :, 2, None] * b[..., None, 2, :]
    return o.astype(F32)


def mul31(a, x):
    a, x = np.asarray(a, F32).astype(F64), np.asarray(x, F32).astype(F64)
    return ((a[..., :, 0] * x[..., None, 0] + a[..., :, 1] * x[..., None, 1]) + a[..., :, 2] * x[..., None, 2]).astype(F32)


def _m9(a):
    a = np.asarray(a, F32).astype(F64)
    return [a[..., i, j] for i in range(3) for j in range(3)]


def det33(a):
    m0, m1, m2, m3, m4, m5, m6, m7, m8 = _m9(a)
    return (m0 * (m4 * m8 - m5 * m7) + m1 * (m5 * m6 - m3 * m8)) + m2 * (m3 * m7 - m4 * m6)


def inv33(a):
    m0, m1, m2, m3, m4, m5, m6, m7, m8 = _m9(a)
    c0, c1, c2 = m4 * m8 - m5 * m7, m5 * m6 - m3 * m8, m3 * m7 - m4 * m6
    det = (m0 * c0 + m1 * c1) + m2 * c2
    with np.errstate(all="ignore"):
        o = [c0 / det, (m2 * m7 - m1 * m8) / det, (m1 * m5 - m2 * m4) / det, c1 / det, (m0 * m8 - m2 * m6) / det, (m2 * m3 - m0 * m5) / det,
             c2 / det, (m1 * m6 - m0 * m7) / det, (m0 * m4 - m1 * m3) / det]
    return np.stack(o, -1).reshape(np.shape(a)).astype(F32)


def unit3(v):
    v = np.asarray(v, F32).astype(F64)
    n = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    with np.errstate(all="ignore"):
        return (v / n[..., None]).astype(F32)


def orient(v):
    """the first component of largest magnitude positive"""
    v = np.array(v)
    k = np.argmax(np.abs(v), axis=1)                               # the first of equal magnitudes
    neg = v[np.arange(len(v)), k] < 0
    v[neg] = -v[neg]
    return v


class Literal:
    kind = "literal"

    @staticmethod
    def null_vector(A):
        """A [B, m, 9] float32 -> the oriented right singular vector of the smallest singular value, float32 [B, 9]"""
        _, V, _, perm = jacobi_batch(A)
        return orient(_col(V, perm[:, 8])).astype(F32)

    @staticmethod
    def rank2(Fpre):
        """u diag(w0, w1, 0) vt of float32 [B, 3, 3]: the two leading terms of G V^T, one narrowing"""
        G, V, _, perm = jacobi_batch(Fpre)
        g0, v0, g1, v1 = _col(G, perm[:, 0]), _col(V, perm[:, 0]), _col(G, perm[:, 1]), _col(V, perm[:, 1])
        return (g0[:, :, None] * v0[:, None, :] + g1[:, :, None] * v1[:, None, :]).astype(F32)

    @staticmethod
    def svd33(a):
        """float32 3x3 -> u (by column), w descending, vt (by row), float32"""
        G, V, sig, perm = jacobi_batch(np.asarray(a, F32)[None])
        p = perm[0]
        with np.errstate(all="ignore"):
            u = (G[0][:, p] / sig[0][p][None, :]).astype(F32)
        return u, sig[0][p].astype(F32), V[0][:, p].T.astype(F32)

    @staticmethod
    def tri_null(A):
        """A [B, 4, 4] float32 -> vt.row(3) as float32 [B, 4]"""
        _, V, _, perm = jacobi_batch(A)
        return _col(V, perm[:, 3]).astype(F32)

    mul33, mul31, inv33, det33, unit3 = staticmethod(mul33), staticmethod(mul31), staticmethod(inv33), staticmethod(det33), staticmethod(unit3)


class Independent:
    kind = "independent"

    @staticmethod
    def null_vector(A):
        return orient(np.linalg.svd(np.asarray(A, F32).astype(F64))[2][:, -1, :]).astype(F32)

    @staticmethod
    def rank2(Fpre):
        u, w, vt = np.linalg.svd(np.asarray(Fpre, F32).astype(F64))
        w[:, 2] = 0
        return (u @ (w[:, :, None] * vt)).astype(F32)

    @staticmethod
    def svd33(a):
        u, w, vt = np.linalg.svd(np.asarray(a, F32).astype(F64))
        return u.astype(F32), w.astype(F32), vt.astype(F32)

    @staticmethod
    def tri_null(A):
        return np.linalg.svd(np.asarray(A, F32).astype(F64))[2][:, -1, :].astype(F32)

    @staticmethod
    def mul33(a, b):
        return (np.asarray(a, F32).astype(F64) @ np.asarray(b, F32).astype(F64)).astype(F32)

    @staticmethod
    def mul31(a, x):
        return np.einsum("...ij,...j->...i", np.asarray(a, F32).astype(F64), np.asarray(x, F32).astype(F64)).astype(F32)

    @staticmethod
    def inv33(a):
        a = np.asarray(a, F32).astype(F64)
        try:
            return np.linalg.inv(a).astype(F32)
        except np.linalg.LinAlgError:
            return np.full(a.shape, np.nan, F32)

    @staticmethod
    def det33(a):
        return np.linalg.det(np.asarray(a, F32).astype(F64))

    @staticmethod
    def unit3(v):
        v = np.asarray(v, F32).astype(F64)
        with np.errstate(all="ignore"):
            return (v / np.linalg.norm(v, axis=-1)[..., None]).astype(F32)


# ---------------------------------------------------------------- Normalize (:761-807)
def normalize(xy):
    """xy float32 [n, 2] -> (normalised points [n, 2], T 3x3, (meanX, meanY, sX, sY)); every sum float32 in key order"""
    xy = np.asarray(xy, F32).reshape(-1, 2)
    n = len(xy)
    with np.errstate(all="ignore"):
        mean = (np.cumsum(xy, axis=0, dtype=F32)[-1] if n else np.zeros(2, F32)) / F32(n)
        d = xy - mean
        dev = (np.cumsum(np.abs(d), axis=0, dtype=F32)[-1] if n else np.zeros(2, F32)) / F32(n)
        s = F32(1) / dev
    T = np.eye(3, dtype=F32)
    T[0, 0], T[1, 1], T[0, 2], T[1, 2] = s[0], s[1], -mean[0] * s[0], -mean[1] * s[1]
    return d * s, T, (mean[0], mean[1], s[0], s[1])


# ---------------------------------------------------------------- ComputeH21 / ComputeF21 (:239-316), batched over hypotheses
def system_h(p1, p2):
    """p1, p2 float32 [B, 8, 2] -> A [B, 16, 9]"""
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    z, o = np.zeros_like(u1), np.ones_like(u1)
    even = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], -1)
    odd = np.stack([u1, v1, o, z, z, z, -u2 * u1, -u2 * v1, -u2], -1)
    return np.stack([even, odd], 2).reshape(len(p1), 16, 9).astype(F32)


def system_f(p1, p2):
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    return np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], -1).astype(F32)


def compute_h21(p1, p2, la=Literal):
    return la.null_vector(system_h(p1, p2)).reshape(-1, 3, 3)


def compute_f21(p1, p2, la=Literal):
    return la.rank2(la.null_vector(system_f(p1, p2)).reshape(-1, 3, 3))


# ---------------------------------------------------------------- CheckHomography / CheckFundamental (:318-481): chi-squares [B, N], the source's expressions
def chi_h(H21, H12, x1, x2, inv_s2):
    h, g = [H21[:, i, j, None] for i in range(3) for j in range(3)], [H12[:, i, j, None] for i in range(3) for j in range(3)]
    u1, v1, u2, v2 = x1[None, :, 0], x1[None, :, 1], x2[None, :, 0], x2[None, :, 1]
    with np.errstate(all="ignore"):
        w2 = F32(1) / (g[6] * u2 + g[7] * v2 + g[8])
        a, b = (g[0] * u2 + g[1] * v2 + g[2]) * w2, (g[3] * u2 + g[4] * v2 + g[5]) * w2
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv_s2
        w1 = F32(1) / (h[6] * u1 + h[7] * v1 + h[8])
        a, b = (h[0] * u1 + h[1] * v1 + h[2]) * w1, (h[3] * u1 + h[4] * v1 + h[5]) * w1
        chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv_s2
    return chi1, chi2


def chi_f(F21, x1, x2, inv_s2):
    f = [F21[:, i, j, None] for i in range(3) for j in range(3)]
    u1, v1, u2, v2 = x1[None, :, 0], x1[None, :, 1], x2[None, :, 0], x2[None, :, 1]
    with np.errstate(all="ignore"):
        a2, b2, c2 = f[0] * u1 + f[1] * v1 + f[2], f[3] * u1 + f[4] * v1 + f[5], f[6] * u1 + f[7] * v1 + f[8]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_s2
        a1, b1, c1 = f[0] * u2 + f[3] * v2 + f[6], f[1] * u2 + f[4] * v2 + f[7], f[2] * u2 + f[5] * v2 + f[8]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_s2
    return chi1, chi2


def score_of(chi1, chi2, th, th_score=F32(5.991)):
    """the sequential loop over the matches, vectorised over the hypotheses: (scores [B], masks [B, N])"""
    B, N = chi1.shape
    score = np.zeros(B, F32)
    with np.errstate(all="ignore"):
        for i in range(N):
            out1, out2 = chi1[:, i] > th, chi2[:, i] > th
            score = np.where(out1, score, score + (th_score - chi1[:, i]))
            score = np.where(out2, score, score + (th_score - chi2[:, i]))
    return score.astype(F32), ~((chi1 > th) | (chi2 > th))


def first_best(scores):
    """currentScore > score from score = 0: (the first iteration of the largest score above 0 or -1, that score or 0)"""
    best, it = F32(0), -1
    for k, s in enumerate(scores):
        if s > best:
            best, it = s, k
    return it, best


# ---------------------------------------------------------------- the motions
def k33(cam):
    fx, fy, cx, cy = [F32(c) for c in cam]
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F32)


def motions_h(H21, cam, la=Literal):
    """ReconstructH :597-700 -> (R [8, 3, 3], t [8, 3]) or None where the d1/d2, d2/d3 gate returns false"""
    K = k33(cam)
    A = la.mul33(la.mul33(la.inv33(K), H21), K)
    U, w, Vt = la.svd33(A)
    s = F32(la.det33(U) * la.det33(Vt))
    d1, d2, d3 = w
    with np.errstate(all="ignore"):
        if float(d1 / d2) < 1.00001 or float(d2 / d3) < 1.00001:
            return None
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
        aux_stheta = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
        ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        stheta = [aux_stheta, -aux_stheta, -aux_stheta, aux_stheta]
        aux_sphi = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
        cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sphi = [aux_sphi, -aux_sphi, -aux_sphi, aux_sphi]
        Rs, ts = [], []
        for m in range(8):
            i = m & 3
            Rp = np.eye(3, dtype=F32)
            if m < 4:
                Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ctheta, -stheta[i], stheta[i], ctheta
                tp = np.array([x1[i] * (d1 - d3), F32(0) * (d1 - d3), -x3[i] * (d1 - d3)], F32)
            else:
                Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cphi, sphi[i], -1, sphi[i], -cphi
                tp = np.array([x1[i] * (d1 + d3), F32(0) * (d1 + d3), x3[i] * (d1 + d3)], F32)
            Rs.append(s * la.mul33(la.mul33(U, Rp), Vt))
            ts.append(la.unit3(la.mul31(U, tp)))
    return np.array(Rs, F32), np.array(ts, F32)


def motions_f(F21, cam, la=Literal):
    """ReconstructF :492-510 with DecomposeE -> (R [4, 3, 3], t [4, 3]) in the order (R1, t), (R2, t), (R1, -t), (R2, -t)"""
    K = k33(cam)
    E = la.mul33(la.mul33(K.T.copy(), F21), K)
    u, _, vt = la.svd33(E)
    t = la.unit3(u[:, 2])
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F32)
    R1 = la.mul33(la.mul33(u, W), vt)
    if la.det33(R1) < 0:
        R1 = -R1
    R2 = la.mul33(la.mul33(u, W.T.copy()), vt)
    if la.det33(R2) < 0:
        R2 = -R2
    return np.array([R1, R2, R1, R2], F32), np.array([t, t, -t, -t], F32)


# ---------------------------------------------------------------- CheckRT (:810-921), vectorised over the inlier matches
def check_rt(R, t, x1, x2, cam, th2, la=Literal):
    """x1, x2 float32 [n, 2]: the inlier matches -> (code [n]: 0 rejected, 1 accepted, 2 accepted and good; X [n, 3]; cos [n])"""
    n = len(x1)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros((0, 3), F32), np.zeros(0, F32)
    fx, fy, cx, cy = [F32(c) for c in cam]
    K = k33(cam)
    P1 = np.zeros((3, 4), F32)
    P1[:, :3] = K
    Rt = np.concatenate([np.asarray(R, F32), np.asarray(t, F32).reshape(3, 1)], 1).astype(F64)
    Kd = K.astype(F64)
    P2 = ((Kd[:, 0, None] * Rt[None, 0, :] + Kd[:, 1, None] * Rt[None, 1, :]) + Kd[:, 2, None] * Rt[None, 2, :]).astype(F32)
    O2 = -la.mul31(np.asarray(R, F32).T.copy(), t)
    u1, v1, u2, v2 = x1[:, 0, None], x1[:, 1, None], x2[:, 0, None], x2[:, 1, None]
    with np.errstate(all="ignore"):
        A = np.stack([u1 * P1[2] - P1[0], v1 * P1[2] - P1[1], u2 * P2[2] - P2[0], v2 * P2[2] - P2[1]], 1).astype(F32)
        x = la.tri_null(A)
        X = (x[:, :3] / x[:, 3, None]).astype(F32)
        finite = np.isfinite(X).all(1)
        Xd = X.astype(F64)
        dist1 = np.sqrt((Xd[:, 0] * Xd[:, 0] + Xd[:, 1] * Xd[:, 1]) + Xd[:, 2] * Xd[:, 2]).astype(F32)
        n2 = (X - O2[None, :]).astype(F32)
        nd = n2.astype(F64)
        dist2 = np.sqrt((nd[:, 0] * nd[:, 0] + nd[:, 1] * nd[:, 1]) + nd[:, 2] * nd[:, 2]).astype(F32)
        dot = (Xd[:, 0] * nd[:, 0] + Xd[:, 1] * nd[:, 1]) + Xd[:, 2] * nd[:, 2]
        cosp = (dot / (dist1 * dist2).astype(F64)).astype(F32)
        low = cosp.astype(F64) < 0.99998
        Rd, td = np.asarray(R, F32).astype(F64), np.asarray(t, F32).astype(F64)
        X2 = np.stack([(((Rd[i, 0] * Xd[:, 0] + Rd[i, 1] * Xd[:, 1]) + Rd[i, 2] * Xd[:, 2]) + td[i]) for i in range(3)], 1).astype(F32)
        ok = finite & ~((X[:, 2] <= 0) & low) & ~((X2[:, 2] <= 0) & low)
        invZ1 = F32(1) / X[:, 2]
        im1x, im1y = fx * X[:, 0] * invZ1 + cx, fy * X[:, 1] * invZ1 + cy
        e1 = (im1x - x1[:, 0]) * (im1x - x1[:, 0]) + (im1y - x1[:, 1]) * (im1y - x1[:, 1])
        ok &= ~(e1 > th2)
        invZ2 = F32(1) / X2[:, 2]
        im2x, im2y = fx * X2[:, 0] * invZ2 + cx, fy * X2[:, 1] * invZ2 + cy
        e2 = (im2x - x2[:, 0]) * (im2x - x2[:, 0]) + (im2y - x2[:, 1]) * (im2y - x2[:, 1])
        ok &= ~(e2 > th2)
    code = np.where(ok, np.where(low, 2, 1), 0)
    return code, X, cosp


def selected_cosine(cosines, min_triangulated):
    """vCosParallax sorted, element min(minTriangulated, size - 1) (quirk 5)"""
    c = np.sort(np.asarray(cosines, F32))
    return c[min(min_triangulated, len(c) - 1)]


# ---------------------------------------------------------------- the two decisions (:512-582, :702-743)
def decide_f(n_good, parallax_ok, N, min_tri, min_frac):
    """parallax_ok[m]: parallax_m > minParallax.  -> (the motion handed out or -1, the motion that decided or -1)"""
    max_good = max(n_good[:4])
    n_min_good = max(int(F32(min_frac) * F32(N)), min_tri)
    nsimilar = sum(1 for g in n_good[:4] if g > 0.7 * max_good)
    if max_good < n_min_good or nsimilar > 1:
        return -1, -1
    for m in range(4):
        if max_good == n_good[m]:
            return (m if parallax_ok[m] else -1), m
    return -1, -1


def decide_h(n_good, parallax_ok, N, min_tri, min_frac):
    """parallax_ok[m]: parallax_m >= minParallax"""
    best, second, idx = 0, 0, -1
    for m in range(8):
        if n_good[m] > best:
            second, best, idx = best, n_good[m], m
        elif n_good[m] > second:
            second = n_good[m]
    if idx < 0:
        return -1, -1
    ok = second < 0.75 * best and parallax_ok[idx] and best > min_tri and F32(best) > F32(min_frac) * F32(N)
    return (idx if ok else -1), idx


# ---------------------------------------------------------------- MonoEstimator::Initialize
def estimate(kps1, kps2, matches12, params=None, draws=None, kind="literal"):
    with np.errstate(all="ignore"):
        return _estimate(kps1, kps2, matches12, params, draws, kind)


def _estimate(kps1, kps2, matches12, params, draws, kind):
    la = Literal if kind == "literal" else Independent
    P = dict(DEFAULT)
    P.update(params or {})
    cam = (P["fx"], P["fy"], P["cx"], P["cy"])
    xy1, xy2 = np.asarray(kps1, F32).reshape(-1, 2), np.asarray(kps2, F32).reshape(-1, 2)
    n1, n2 = len(xy1), len(xy2)
    matches12 = np.asarray(matches12, np.int64).reshape(-1)
    i1 = np.nonzero((matches12 >= 0) & (matches12 < n2))[0]
    i2 = matches12[i1]
    N, H = len(i1), int(P["max_iterations"])
    out = dict(status=TOO_FEW, n_matches=N, model=MODEL_NONE, best_solution=0, best_it_h=0, best_it_f=0, n_triangulated=0, score_h=F32(0), score_f=F32(0), rh=F32(0),
               cos_parallax=F32(0), H21=np.zeros(9, F32), F21=np.zeros(9, F32), n_good=np.zeros(8, np.int32), R21=np.zeros(9, F32), t21=np.zeros(3, F32),
               inliers_h=np.zeros(n1, np.uint8), inliers_f=np.zeros(n1, np.uint8), p3d=np.zeros((n1, 3), F32), triangulated=np.zeros(n1, np.uint8), hyp=None,
               i1=i1, i2=i2, parallax_deg=0.0)
    if N < 8:
        return out
    out.update(status=FAILED, best_solution=-1, cos_parallax=F32(1))
    pn1, T1, _ = normalize(xy1)
    pn2, T2, _ = normalize(xy2)
    T2inv, T2t = la.inv33(T2), T2.T.copy()
    sets = np.array(sample_sets(N, H, int(P["seed"]), draws), np.int64).reshape(H, 8)
    a, b = pn1[i1[sets]], pn2[i2[sets]]
    x1, x2 = xy1[i1], xy2[i2]
    sigma = F32(P["sigma"])
    inv_s2 = F32(1) / (sigma * sigma)
    H21 = la.mul33(la.mul33(T2inv[None], compute_h21(a, b, la)), T1[None])
    H12 = la.inv33(H21)
    F21 = la.mul33(la.mul33(T2t[None], compute_f21(a, b, la)), T1[None])
    ch1, ch2 = chi_h(H21, H12, x1, x2, inv_s2)
    cf1, cf2 = chi_f(F21, x1, x2, inv_s2)
    sh, mh = score_of(ch1, ch2, F32(5.991))
    sf, mf = score_of(cf1, cf2, F32(3.841))
    out["hyp"] = dict(sets=sets, H21=H21, F21=F21, score_h=sh, score_f=sf, chi=(ch1, ch2, cf1, cf2))
    bh, SH = first_best(sh)
    bf, SF = first_best(sf)
    out.update(best_it_h=bh, best_it_f=bf, score_h=SH, score_f=SF)
    if bh >= 0:
        out["H21"], out["inliers_h"][:N] = H21[bh].reshape(9), mh[bh]
    if bf >= 0:
        out["F21"], out["inliers_f"][:N] = F21[bf].reshape(9), mf[bf]
    with np.errstate(all="ignore"):
        rh = SH / (SH + SF)
    out["rh"] = rh
    model = MODEL_H if float(rh) > 0.40 else MODEL_F
    if (model == MODEL_F and bf < 0) or (model == MODEL_H and bh < 0):
        return out                                                  # quirk 2: the mask is empty and F21 an empty Mat; the library fails
    out["model"] = model
    mask = (out["inliers_h"] if model == MODEL_H else out["inliers_f"])[:N] != 0
    n_in = int(mask.sum())
    if model == MODEL_H:
        mo = motions_h(out["H21"].reshape(3, 3), cam, la)
        if mo is None:
            return out
    else:
        mo = motions_f(out["F21"].reshape(3, 3), cam, la)
    Rs, ts = mo
    th2 = F32(4.0 * float(sigma * sigma))
    cmin, n_good, cosk, runs = cos_min_parallax(P["min_parallax_deg"]), [0] * 8, [F32(1)] * 8, []
    for m in range(len(Rs)):
        code, X, cosp = check_rt(Rs[m], ts[m], x1[mask], x2[mask], cam, th2, la)
        runs.append((code, X))
        n_good[m] = int((code == 2).sum())
        if n_good[m] > 0:
            cosk[m] = selected_cosine(cosp[code > 0], int(P["min_triangulated"]))
    if kind == "literal":                                          # D21
        strict, loose = [n_good[m] > 0 and cosk[m] < cmin for m in range(8)], [n_good[m] > 0 and cosk[m] <= cmin for m in range(8)]
    else:                                                          # the source: degrees through acos
        deg = [math.acos(max(-1.0, min(1.0, float(cosk[m])))) * 180 / math.pi if n_good[m] > 0 else 0.0 for m in range(8)]
        strict, loose = [d > float(P["min_parallax_deg"]) for d in deg], [d >= float(P["min_parallax_deg"]) for d in deg]
    win, dec = (decide_h(n_good, loose, n_in, int(P["min_triangulated"]), P["min_frac_triangulated"]) if model == MODEL_H
                else decide_f(n_good, strict, n_in, int(P["min_triangulated"]), P["min_frac_triangulated"]))
    out["n_good"] = np.array(n_good, np.int32)
    out["best_solution"] = dec
    out["cos_parallax"] = cosk[dec] if dec >= 0 else F32(1)
    out["motions"] = (Rs, ts)
    out["n_inliers_model"] = n_in
    if win < 0:
        return out
    code, X = runs[win]
    idx = i1[mask]
    out["p3d"][idx[code > 0]] = X[code > 0]
    out["triangulated"][idx[code == 2]] = 1
    out["R21"], out["t21"], out["n_triangulated"] = Rs[win].reshape(9).copy(), ts[win].copy(), n_good[win]
    finite = np.isfinite(out["R21"]).all() and np.isfinite(out["t21"]).all()
    out["status"] = NONFINITE if not finite else OK_H if model == MODEL_H else OK_F
    return out
