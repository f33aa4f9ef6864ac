"""Reference for the batched EPnP RANSAC (PnPsolver, src/estimators/PnPsolver.cc), twice.

LITERAL      numpy float64 SCALARS, one IEEE operation per Python operation in the order the reference writes them, np.float32 where the
             reference narrows; every decomposition is the one-sided cyclic Jacobi SVD of DESIGN.md D17; the draws are those of D18; the RANSAC
             loop is `iterate` as it is written (ransac_literal).  The sums over the points of an EPnP run in the order `order` gives: None is point
             order, which is the reference's order AND the device's (every such sum is one lane's), a permutation is one of
             the seeded orders the cases' qualification runs.
INDEPENDENT  the same EPnP with numpy.linalg for every decomposition and vectorised sums, and the RANSAC in the closed "records" form
             (ransac_records): Refine() is a pure function of the best set, so it is evaluated once per strict prefix maximum of the counts.
             Solver(kind="independent") runs every Refine() through it; its minimal-set hypotheses are LITERAL's (see below).

A minimal-set hypothesis takes its four vectors from the null space of MtM (dimension >= 4 with 4 points): the basis is the decomposition's, so
LITERAL and INDEPENDENT agree on such a hypothesis only by accident.  They are compared on the refine poses, where the four smallest eigenvalues
are apart (the cases carry pixel noise for that).
"""
import numpy as np

F32, F64 = np.float32, np.float64
EPS = F64(np.finfo(np.float64).eps)
SVD_SWEEPS = 30
MAX_SET = 16
TOO_FEW, REFINED, BEST, NONE, NONFINITE = 0, 1, 2, 3, 4
CORR_DTYPE = np.dtype([("Xw", "<f4", 3), ("u", "<f4"), ("v", "<f4"), ("sigma2", "<f4"), ("kp", "<i4"), ("_pad", "<i4")])
DEFAULT = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991)      # Tracking_datastructs.cc:53-58


# ---------------------------------------------------------------- SetRansacParameters (:127-163)
def plan(N, probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, **_):
    """(effective min_inliers, epsilon as float32, max_iterations)"""
    import math
    eps = F32(epsilon)
    with np.errstate(all="ignore"):
        prod = F32(N) * eps                                        # int x float
        n_min = int(prod) if np.isfinite(prod) else 0              # truncated
        n_min = max(n_min, min_inliers, min_set)
        ratio = F32(n_min) / F32(N)
        if eps < ratio:
            eps = ratio
        if n_min == N:
            its = 1
        else:
            e = float(eps)
            try:
                x = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(e, 3)))      # the exponent is 3 although the set is 4
            except (ValueError, ZeroDivisionError, OverflowError):
                x = 1
            its = max(1, x)
    return n_min, eps, max(1, min(its, max_iterations))


# ---------------------------------------------------------------- the draws
_M64 = (1 << 64) - 1


def mix(c):
    z = (0x9E3779B97F4A7C15 * ((c + 1) & _M64)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def draw32(seed, it, k, min_set, draws=None):
    """the 32-bit word draw k of absolute iteration `it` reduces: a table row overrides the generator"""
    if draws is not None and it < len(draws):
        return int(draws[it][k])
    return mix((seed + it * min_set + k) & _M64) >> 32


def sample(N, min_set, words):
    """min_set draws without replacement (:194-207): take avail[randi], move the back element into its place, pop"""
    avail = list(range(N))
    out = []
    for k in range(min_set):
        randi = (int(words[k]) * len(avail)) >> 32
        out.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return out


# ---------------------------------------------------------------- the one decomposition, LITERAL
def jacobi_svd(A):
    """one-sided cyclic Jacobi SVD of A (m x n): returns (G = U Sigma, V, sig by column, perm: rank -> column)"""
    G = np.array(A, F64)
    m, n = G.shape
    V = np.eye(n, dtype=F64)
    f2 = F64(0)
    for e in G.reshape(-1):
        f2 = f2 + e * e
    tiny = (F64(n) * EPS) * (F64(n) * EPS) * f2
    for _ in range(SVD_SWEEPS):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                a = b = g = F64(0)
                cp, cq = G[:, p], G[:, q]
                for i in range(m):
                    gp, gq = cp[i], cq[i]
                    a = a + gp * gp
                    b = b + gq * gq
                    g = g + gp * gq
                if not (a > tiny) or not (b > tiny) or not (abs(g) > EPS * np.sqrt(a * b)):
                    continue
                zeta = (b - a) / (F64(2) * g)
                t = (F64(-1) if zeta < 0 else F64(1)) / (abs(zeta) + np.sqrt(F64(1) + zeta * zeta))
                c = F64(1) / np.sqrt(F64(1) + t * t)
                s = c * t
                for M in (G, V):                                   # elementwise: one multiply, one multiply, one add per entry
                    x, y = M[:, p].copy(), M[:, q].copy()
                    M[:, p] = c * x - s * y
                    M[:, q] = s * x + c * y
                rotated = True
        if not rotated:
            break
    sig = np.zeros(n, F64)
    for j in range(n):
        s = F64(0)
        for i in range(m):
            s = s + G[i, j] * G[i, j]
        sig[j] = np.sqrt(s)
    perm = []
    for j in range(n):                                             # stable insertion sort, descending
        k = len(perm)
        while k > 0 and sig[perm[k - 1]] < sig[j]:
            k -= 1
        perm.insert(k, j)
    return G, V, sig, perm


def _cut(sig, perm):
    s = F64(0)
    for c in perm:
        s = s + sig[c]
    return F64(2) * EPS * s


def pinv_solve(A, b):
    G, V, sig, perm = jacobi_svd(A)
    m, n = G.shape
    cut = _cut(sig, perm)
    x = np.zeros(n, F64)
    for c in perm:
        if not (sig[c] > cut):
            continue
        d = F64(0)
        for j in range(m):
            d = d + (G[j, c] / sig[c]) * b[j]
        for i in range(n):
            x[i] = x[i] + V[i, c] * (d / sig[c])
    return x


def pinv3(A):
    G, V, sig, perm = jacobi_svd(A)
    cut = _cut(sig, perm)
    out = np.zeros((3, 3), F64)
    for i in range(3):
        for j in range(3):
            acc = F64(0)
            for c in perm:
                if not (sig[c] > cut):
                    continue
                acc = acc + V[i, c] * ((G[j, c] / sig[c]) / sig[c])
            out[i, j] = acc
    return out


# ---------------------------------------------------------------- EPnP (:381-956), LITERAL
class Margins:
    """the smallest relative margin by which a decision of each kind was taken (the cases' qualification)"""

    def __init__(self):
        self.m = {}

    def note(self, kind, value):
        v = float(value)
        if not np.isfinite(v):
            return
        self.m[kind] = min(self.m.get(kind, np.inf), v)

    def merge(self, other):
        for k, v in other.m.items():
            self.note(k, v)

    def smallest(self):
        return min(self.m.values()) if self.m else np.inf


def _dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _dist2(p1, p2):
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2])


def _sign_margin(mg, kind, x, scale):
    if mg is not None:
        with np.errstate(all="ignore"):
            mg.note(kind, abs(x) / scale if scale > 0 else np.inf)


def _qr_solve(A, b, X):
    """qr_solve (:866-956) on a 6x4 system, in place; leaves X alone when a column is zero"""
    nr, nc = 6, 4
    pA = A.reshape(-1)
    A1, A2 = np.zeros(4, F64), np.zeros(4, F64)
    for k in range(nc):
        kk = k * (nc + 1)
        ik = kk
        eta = abs(pA[ik])
        for i in range(k + 1, nr):                                 # as written: the element is read before the pointer moves
            elt = abs(pA[ik])
            if eta < elt:
                eta = elt
            ik += nc
        if eta == 0:
            return
        ik = kk
        s = F64(0)
        inv_eta = F64(1) / eta
        for i in range(k, nr):
            pA[ik] = pA[ik] * inv_eta
            s = s + pA[ik] * pA[ik]
            ik += nc
        sigma = np.sqrt(s)
        if pA[kk] < 0:
            sigma = -sigma
        pA[kk] = pA[kk] + sigma
        A1[k] = sigma * pA[kk]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            ik, s2 = kk, F64(0)
            for i in range(k, nr):
                s2 = s2 + pA[ik] * pA[ik + j - k]
                ik += nc
            tau = s2 / A1[k]
            ik = kk
            for i in range(k, nr):
                pA[ik + j - k] = pA[ik + j - k] - tau * pA[ik]
                ik += nc
    for j in range(nc):
        jj = j * (nc + 1)
        ij, tau = jj, F64(0)
        for i in range(j, nr):
            tau = tau + pA[ij] * b[i]
            ij += nc
        tau = tau / A1[j]
        ij = jj
        for i in range(j, nr):
            b[i] = b[i] - tau * pA[ij]
            ij += nc
    X[nc - 1] = b[nc - 1] / A2[nc - 1]
    for i in range(nc - 2, -1, -1):
        ij, s = i * nc + (i + 1), F64(0)
        for j in range(i + 1, nc):
            s = s + pA[ij] * X[j]
            ij += 1
        X[i] = (b[i] - s) / A2[i]


def _gauss_newton(L, rho, betas):
    x = np.zeros(4, F64)                                           # the reference leaves it unset before the first qr_solve: zero here
    two = F64(2)
    for _ in range(5):
        A, b = np.zeros((6, 4), F64), np.zeros(6, F64)
        for i in range(6):
            r = L[i]
            A[i, 0] = two * r[0] * betas[0] + r[1] * betas[1] + r[3] * betas[2] + r[6] * betas[3]
            A[i, 1] = r[1] * betas[0] + two * r[2] * betas[1] + r[4] * betas[2] + r[7] * betas[3]
            A[i, 2] = r[3] * betas[0] + r[4] * betas[1] + two * r[5] * betas[2] + r[8] * betas[3]
            A[i, 3] = r[6] * betas[0] + r[7] * betas[1] + r[8] * betas[2] + two * r[9] * betas[3]
            b[i] = rho[i] - (r[0] * betas[0] * betas[0] + r[1] * betas[0] * betas[1] + r[2] * betas[1] * betas[1] + r[3] * betas[0] * betas[2] +
                             r[4] * betas[1] * betas[2] + r[5] * betas[2] * betas[2] + r[6] * betas[0] * betas[3] + r[7] * betas[1] * betas[3] +
                             r[8] * betas[2] * betas[3] + r[9] * betas[3] * betas[3])
        _qr_solve(A, b, x)
        for i in range(4):
            betas[i] = betas[i] + x[i]


def epnp_literal(pts, cam, order=None, margins=None):
    """compute_pose (:483-531).  pts: (n, 5) float64 rows Xw, Yw, Zw, u, v; cam = (fu, fv, uc, vc).  Returns (R (3, 3), t (3,)) in float64."""
    with np.errstate(all="ignore"):
        return _epnp_literal(np.asarray(pts, F64), [F64(c) for c in cam], order, margins)


def _epnp_literal(P, cam, order, mg):
    fu, fv, uc, vc = cam
    n = len(P)
    seq = range(n) if order is None else [int(i) for i in order]
    dn = F64(n)
    cws = np.zeros((4, 3), F64)
    for j in range(3):                                             # choose_control_points
        s = F64(0)
        for i in seq:
            s = s + P[i, j]
        cws[0, j] = s / dn
    pca = np.zeros((3, 3), F64)
    for i in seq:
        d = P[i, :3] - cws[0]
        pca = pca + np.outer(d, d)
    _, V, sig, perm = jacobi_svd(pca)
    for i in range(1, 4):
        c = perm[i - 1]
        k = np.sqrt(sig[c] / dn)
        big = 0                                                    # D17: an axis points where its component of largest magnitude is positive
        for j in (1, 2):
            if abs(V[j, c]) > abs(V[big, c]):
                big = j
        sgn = F64(-1) if V[big, c] < 0 else F64(1)
        for j in range(3):
            cws[i, j] = cws[0, j] + k * (sgn * V[j, c])
    rho = np.array([_dist2(cws[0], cws[1]), _dist2(cws[0], cws[2]), _dist2(cws[0], cws[3]), _dist2(cws[1], cws[2]), _dist2(cws[1], cws[3]),
                    _dist2(cws[2], cws[3])], F64)
    cc = np.zeros((3, 3), F64)
    for i in range(3):
        for j in range(1, 4):
            cc[i, j - 1] = cws[j, i] - cws[0, i]
    ci = pinv3(cc)                                                 # compute_barycentric_coordinates
    al = np.zeros((n, 4), F64)
    for i in range(n):
        d0, d1, d2 = P[i, 0] - cws[0, 0], P[i, 1] - cws[0, 1], P[i, 2] - cws[0, 2]
        for j in range(3):
            al[i, 1 + j] = ci[j, 0] * d0 + ci[j, 1] * d1 + ci[j, 2] * d2
        al[i, 0] = F64(1) - al[i, 1] - al[i, 2] - al[i, 3]
    mtm = np.zeros((12, 12), F64)                                  # fill_M and MtM: the rows of M in order, every product formed (zeros too)
    for i in seq:
        m1, m2 = np.zeros(12, F64), np.zeros(12, F64)
        for k in range(4):
            m1[3 * k], m1[3 * k + 2] = al[i, k] * fu, al[i, k] * (uc - P[i, 3])
            m2[3 * k + 1], m2[3 * k + 2] = al[i, k] * fv, al[i, k] * (vc - P[i, 4])
        mtm = mtm + np.outer(m1, m1)
        mtm = mtm + np.outer(m2, m2)
    _, V12, sig12, perm12 = jacobi_svd(mtm)
    ut = np.stack([V12[:, perm12[r]] for r in range(12)])         # row r = the right singular vector of rank r
    v = [ut[11], ut[10], ut[9], ut[8]]
    dv = np.zeros((4, 6, 3), F64)                                  # compute_L_6x10
    for i in range(4):
        a, b = 0, 1
        for j in range(6):
            for c in range(3):
                dv[i, j, c] = v[i][3 * a + c] - v[i][3 * b + c]
            b += 1
            if b > 3:
                a += 1
                b = a + 1
    L = np.zeros((6, 10), F64)
    two = F64(2)
    for i in range(6):
        L[i] = [_dot3(dv[0, i], dv[0, i]), two * _dot3(dv[0, i], dv[1, i]), _dot3(dv[1, i], dv[1, i]), two * _dot3(dv[0, i], dv[2, i]),
                two * _dot3(dv[1, i], dv[2, i]), _dot3(dv[2, i], dv[2, i]), two * _dot3(dv[0, i], dv[3, i]), two * _dot3(dv[1, i], dv[3, i]),
                two * _dot3(dv[2, i], dv[3, i]), _dot3(dv[3, i], dv[3, i])]
    Rs, ts, rep = [None] * 4, [None] * 4, [None] * 4
    for var in (1, 2, 3):
        cols = {1: [0, 1, 3, 6], 2: [0, 1, 2], 3: [0, 1, 2, 3, 4]}[var]
        bb = pinv_solve(L[:, cols], rho)
        scale = np.max(np.abs(bb))
        betas = np.zeros(4, F64)
        _sign_margin(mg, "beta_v%d_b0" % var, bb[0], scale)       # one key per variant and coefficient: which rules clear the margin is told apart
        if var == 1:                                               # find_betas_approx_1
            if bb[0] < 0:
                betas[0] = np.sqrt(-bb[0]); betas[1] = -bb[1] / betas[0]; betas[2] = -bb[2] / betas[0]; betas[3] = -bb[3] / betas[0]
            else:
                betas[0] = np.sqrt(bb[0]); betas[1] = bb[1] / betas[0]; betas[2] = bb[2] / betas[0]; betas[3] = bb[3] / betas[0]
        else:                                                      # find_betas_approx_2 and _3
            _sign_margin(mg, "beta_v%d_b2" % var, bb[2], scale)
            _sign_margin(mg, "beta_v%d_b1" % var, bb[1], scale)
            if bb[0] < 0:
                betas[0] = np.sqrt(-bb[0]); betas[1] = np.sqrt(-bb[2]) if bb[2] < 0 else F64(0)
            else:
                betas[0] = np.sqrt(bb[0]); betas[1] = np.sqrt(bb[2]) if bb[2] > 0 else F64(0)
            if bb[1] < 0:
                betas[0] = -betas[0]
            betas[2] = bb[3] / betas[0] if var == 3 else F64(0)
            betas[3] = F64(0)
        _gauss_newton(L, rho, betas)
        ccs = np.zeros((4, 3), F64)                                # compute_ccs
        for i in range(4):
            vv = ut[11 - i]
            for j in range(4):
                for c in range(3):
                    ccs[j, c] = ccs[j, c] + betas[i] * vv[3 * j + c]

        def pc_of(i):
            a = al[i]
            return np.array([a[0] * ccs[0, j] + a[1] * ccs[1, j] + a[2] * ccs[2, j] + a[3] * ccs[3, j] for j in range(3)], F64)

        pc_first = pc_of(0)                                        # solve_for_sign: pcs[2] only
        _sign_margin(mg, "pc_sign", pc_first[2], np.sqrt(_dot3(pc_first, pc_first)))
        if pc_first[2] < 0:
            ccs = -ccs
        pcs = np.stack([pc_of(i) for i in range(n)])
        pc0, pw0 = np.zeros(3, F64), np.zeros(3, F64)              # estimate_R_and_t
        for j in range(3):
            s, s2 = F64(0), F64(0)
            for i in seq:
                s = s + pcs[i, j]
                s2 = s2 + P[i, j]
            pc0[j], pw0[j] = s / dn, s2 / dn
        abt = np.zeros((3, 3), F64)
        for i in seq:
            abt = abt + np.outer(pcs[i] - pc0, P[i, :3] - pw0)
        G, V3, sig3, perm3 = jacobi_svd(abt)
        U = np.stack([G[:, c] / sig3[c] for c in perm3], 1)
        Vs = np.stack([V3[:, c] for c in perm3], 1)
        R = np.zeros((3, 3), F64)
        for i in range(3):
            for j in range(3):
                R[i, j] = _dot3(U[i], Vs[j])
        det = (R[0, 0] * R[1, 1] * R[2, 2] + R[0, 1] * R[1, 2] * R[2, 0] + R[0, 2] * R[1, 0] * R[2, 1] - R[0, 2] * R[1, 1] * R[2, 0] -
               R[0, 1] * R[1, 0] * R[2, 2] - R[0, 0] * R[1, 2] * R[2, 1])
        _sign_margin(mg, "det_sign", det, F64(1))
        if det < 0:
            R[2] = -R[2]
        t = np.array([pc0[0] - _dot3(R[0], pw0), pc0[1] - _dot3(R[1], pw0), pc0[2] - _dot3(R[2], pw0)], F64)
        sum2 = F64(0)                                              # reprojection_error: a mean of distances, not of squares
        for i in seq:
            pw = P[i]
            Xc, Yc = _dot3(R[0], pw) + t[0], _dot3(R[1], pw) + t[1]
            inv_Zc = F64(1) / (_dot3(R[2], pw) + t[2])
            ue, ve = uc + fu * Xc * inv_Zc, vc + fv * Yc * inv_Zc
            sum2 = sum2 + np.sqrt((pw[3] - ue) * (pw[3] - ue) + (pw[4] - ve) * (pw[4] - ve))
        Rs[var], ts[var], rep[var] = R, t, sum2 / dn
    N = 1
    if rep[2] < rep[1]:
        N = 2
    if mg is not None:
        mg.note("choice", abs(rep[2] - rep[1]) / max(rep[1], rep[2]))
        mg.note("choice", abs(rep[3] - rep[N]) / max(rep[N], rep[3]))
    if rep[3] < rep[N]:
        N = 3
    return Rs[N], ts[N]


def check_inliers(R, t, corrs, cam, th2, margins=None):
    """CheckInliers (:314-345) in its mixed precision: (mask uint8 [N], count)"""
    fu, fv, uc, vc = [F64(c) for c in cam]
    mask = np.zeros(len(corrs), np.uint8)
    with np.errstate(all="ignore"):
        for i, c in enumerate(corrs):
            x, y, z = F64(c["Xw"][0]), F64(c["Xw"][1]), F64(c["Xw"][2])
            Xc = F32(R[0, 0] * x + R[0, 1] * y + R[0, 2] * z + t[0])
            Yc = F32(R[1, 0] * x + R[1, 1] * y + R[1, 2] * z + t[1])
            invZc = F32(F64(1) / (R[2, 0] * x + R[2, 1] * y + R[2, 2] * z + t[2]))
            ue = uc + fu * F64(Xc) * F64(invZc)
            ve = vc + fv * F64(Yc) * F64(invZc)
            distX = F32(F64(c["u"]) - ue)
            distY = F32(F64(c["v"]) - ve)
            error2 = distX * distX + distY * distY
            max_error = F32(c["sigma2"]) * F32(th2)
            if margins is not None:
                margins.note("error2", abs(F64(error2) - F64(max_error)) / F64(max_error))
            mask[i] = 1 if error2 < max_error else 0
    return mask, int(mask.sum())


def points_of(corrs, idx):
    return np.array([[c["Xw"][0], c["Xw"][1], c["Xw"][2], c["u"], c["v"]] for c in corrs[idx]], F64).reshape(-1, 5)


def pose4(R, t):
    T = np.eye(4, dtype=F64)
    T[:3, :3], T[:3, 3] = R, t
    return T


# ---------------------------------------------------------------- EPnP, INDEPENDENT
def epnp_independent(pts, cam):
    P = np.asarray(pts, F64)
    if not np.all(np.isfinite(P)):
        return np.full((3, 3), np.nan), np.full(3, np.nan)
    try:
        with np.errstate(all="ignore"):
            return _epnp_independent(P, cam)
    except np.linalg.LinAlgError:
        return np.full((3, 3), np.nan), np.full(3, np.nan)


def _epnp_independent(P, cam):
    fu, fv, uc, vc = [float(c) for c in cam]
    n = len(P)
    X, uv = P[:, :3], P[:, 3:]
    c0 = X.mean(0)
    w, E = np.linalg.eigh((X - c0).T @ (X - c0))
    E = E * np.where(E[np.abs(E).argmax(0), np.arange(3)] < 0, -1.0, 1.0)      # D17's orientation of the axes
    cws = np.vstack([c0] + [c0 + np.sqrt(max(w[k], 0.0) / n) * E[:, k] for k in (2, 1, 0)])
    al3 = np.linalg.solve((cws[1:] - c0).T, (X - c0).T).T
    al = np.hstack([1.0 - al3.sum(1, keepdims=True), al3])
    M = np.zeros((2 * n, 12))
    for k in range(4):
        M[0::2, 3 * k], M[0::2, 3 * k + 2] = al[:, k] * fu, al[:, k] * (uc - uv[:, 0])
        M[1::2, 3 * k + 1], M[1::2, 3 * k + 2] = al[:, k] * fv, al[:, k] * (vc - uv[:, 1])
    _, Em = np.linalg.eigh(M.T @ M)
    v = [Em[:, 0], Em[:, 1], Em[:, 2], Em[:, 3]]                   # ascending eigenvalues: ut[11], ut[10], ut[9], ut[8]
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    dv = np.array([[vi[3 * a:3 * a + 3] - vi[3 * b:3 * b + 3] for (a, b) in pairs] for vi in v])
    d = lambda i, j: (dv[i] * dv[j]).sum(1)
    L = np.stack([d(0, 0), 2 * d(0, 1), d(1, 1), 2 * d(0, 2), 2 * d(1, 2), d(2, 2), 2 * d(0, 3), 2 * d(1, 3), 2 * d(2, 3), d(3, 3)], 1)
    rho = np.array([((cws[a] - cws[b]) ** 2).sum() for (a, b) in pairs])
    best = None
    with np.errstate(all="ignore"):
        for var, cols in ((1, [0, 1, 3, 6]), (2, [0, 1, 2]), (3, [0, 1, 2, 3, 4])):
            bb = np.linalg.lstsq(L[:, cols], rho, rcond=None)[0]
            be = np.zeros(4)
            if var == 1:
                sgn = -1.0 if bb[0] < 0 else 1.0
                be[0] = np.sqrt(sgn * bb[0]); be[1:] = sgn * bb[1:] / be[0]
            else:
                if bb[0] < 0:
                    be[0] = np.sqrt(-bb[0]); be[1] = np.sqrt(-bb[2]) if bb[2] < 0 else 0.0
                else:
                    be[0] = np.sqrt(bb[0]); be[1] = np.sqrt(bb[2]) if bb[2] > 0 else 0.0
                if bb[1] < 0:
                    be[0] = -be[0]
                if var == 3:
                    be[2] = bb[3] / be[0]
            for _ in range(5):                                     # Gauss-Newton on the 6 distance constraints, least squares per step
                B = np.array([[be[0] * be[0], be[0] * be[1], be[1] * be[1], be[0] * be[2], be[1] * be[2], be[2] * be[2], be[0] * be[3], be[1] * be[3],
                               be[2] * be[3], be[3] * be[3]]])
                J = np.stack([2 * L[:, 0] * be[0] + L[:, 1] * be[1] + L[:, 3] * be[2] + L[:, 6] * be[3],
                              L[:, 1] * be[0] + 2 * L[:, 2] * be[1] + L[:, 4] * be[2] + L[:, 7] * be[3],
                              L[:, 3] * be[0] + L[:, 4] * be[1] + 2 * L[:, 5] * be[2] + L[:, 8] * be[3],
                              L[:, 6] * be[0] + L[:, 7] * be[1] + L[:, 8] * be[2] + 2 * L[:, 9] * be[3]], 1)
                if not np.all(np.isfinite(J)):
                    break
                be = be + np.linalg.lstsq(J, rho - (L * B).sum(1), rcond=None)[0]
            ccs = sum(be[i] * v[i] for i in range(4)).reshape(4, 3)
            pcs = al @ ccs
            if pcs[0, 2] < 0:
                pcs = -pcs
            pc0, pw0 = pcs.mean(0), X.mean(0)
            if not np.all(np.isfinite(pcs)):
                continue
            U, _, Vt = np.linalg.svd((pcs - pc0).T @ (X - pw0))
            R = U @ Vt
            if np.linalg.det(R) < 0:
                R[2] = -R[2]
            t = pc0 - R @ pw0
            Pc = X @ R.T + t
            err = np.sqrt((uv[:, 0] - (uc + fu * Pc[:, 0] / Pc[:, 2])) ** 2 + (uv[:, 1] - (vc + fv * Pc[:, 1] / Pc[:, 2])) ** 2).mean()
            if best is None or err < best[0]:
                best = (err, R, t)
    if best is None:
        return np.full((3, 3), np.nan), np.full(3, np.nan)
    return best[1], best[2]


# ---------------------------------------------------------------- the RANSAC loop, twice, over callbacks
def passes_of(it0, max_its, n):
    """iterations a call of iterate(n) runs when nothing returns early: the loop's condition is an OR (:188)"""
    return max(max_its - it0, n) if it0 < max_its else n


def ransac_literal(state, n, N, min_inliers, max_its, hypothesis, refine):
    """PnPsolver::iterate (:171-264) as it is written.  state: dict(iterations, best_inliers, best) — `best` identifies the best set (None: none);
    hypothesis(it) -> (count, identity) for the ABSOLUTE 0-based iteration; refine(best) -> (ok, payload), called wherever the reference calls
    Refine().  Returns dict(status, at_iteration, payload, refine_calls)."""
    out = dict(status=NONE, at_iteration=0, payload=None, refine_calls=[])
    if N < min_inliers:
        out["status"] = TOO_FEW
        return out
    current = 0
    while state["iterations"] < max_its or current < n:
        current += 1
        state["iterations"] += 1
        count, ident = hypothesis(state["iterations"] - 1)
        if count >= min_inliers:
            if count > state["best_inliers"]:
                state["best_inliers"], state["best"] = count, ident
            out["refine_calls"].append(state["best"])
            ok, payload = refine(state["best"])
            if ok:
                out.update(status=REFINED, at_iteration=state["iterations"], payload=payload)
                return out
    if state["best_inliers"] >= min_inliers:                       # mnIterations >= mRansacMaxIts always holds here
        out["status"] = BEST
    return out


def ransac_records(state, n, N, min_inliers, max_its, hypothesis, refine):
    """The closed form: every hypothesis of the call is evaluated first (as the device does), then the counts are walked in order and Refine() is
    evaluated once per distinct best set.  Same arguments and result as ransac_literal; refine_calls lists the distinct evaluations."""
    out = dict(status=NONE, at_iteration=0, payload=None, refine_calls=[])
    if N < min_inliers:
        out["status"] = TOO_FEW
        return out
    it0 = state["iterations"]
    passes = passes_of(it0, max_its, n)
    hyps = [hypothesis(it0 + j) for j in range(passes)]
    verdict = None                                                 # of the current best set
    for j, (count, ident) in enumerate(hyps):
        if count < min_inliers:
            continue
        if count > state["best_inliers"]:
            state["best_inliers"], state["best"], verdict = count, ident, None
        if verdict is None:
            out["refine_calls"].append(state["best"])
            verdict = refine(state["best"])
        if verdict[0]:
            state["iterations"] = it0 + j + 1
            out.update(status=REFINED, at_iteration=it0 + j + 1, payload=verdict[1])
            return out
    state["iterations"] = it0 + passes
    if state["best_inliers"] >= min_inliers:
        out["status"] = BEST
    return out


# ---------------------------------------------------------------- the solver on correspondences
def _order_words(seed, n):
    return np.array([mix((seed << 20) + i) for i in range(n)], np.uint64)


class Solver:
    """PnPsolver on CORR_DTYPE records.  kind: "literal" or "independent".  order_seed: None = point order (the reference's and the device's), an
    int = a seeded permutation of every sum over the points of a Refine()'s EPnP."""

    def __init__(self, corrs, cam, params=None, draws=None, kind="literal", order_seed=None, margins=None):
        self.corrs = np.ascontiguousarray(corrs, CORR_DTYPE).reshape(-1)
        self.cam = tuple(F32(c) for c in cam)
        self.p = dict(DEFAULT, seed=0)
        self.p.update(params or {})
        self.draws, self.kind, self.order_seed, self.margins = draws, kind, order_seed, margins
        self.N = len(self.corrs)
        self.min_inliers, self.epsilon, self.max_its = plan(self.N, **self.p)
        self.state = dict(iterations=0, best_inliers=0, best=None)
        self.best_Tcw = np.zeros((4, 4), F32)
        self.best_mask = np.zeros(self.N, np.uint8)
        self._hyp, self._ref = {}, {}

    def _epnp(self, idx, refine):
        pts = points_of(self.corrs, idx)
        if self.kind == "independent" and refine:                  # a minimal-set hypothesis is basis-dependent: both kinds take LITERAL's
            return epnp_independent(pts, self.cam)
        order = None
        if refine and self.order_seed is not None:
            order = np.argsort(_order_words(self.order_seed, len(idx)), kind="stable")       # a seeded permutation, the same on every machine
        return epnp_literal(pts, self.cam, order, self.margins)

    def hypothesis(self, it):
        if it not in self._hyp:
            ms = self.p["min_set"]
            idx = sample(self.N, ms, [draw32(self.p["seed"], it, k, ms, self.draws) for k in range(ms)])
            R, t = self._epnp(idx, False)
            mask, cnt = check_inliers(R, t, self.corrs, self.cam, self.p["th2"], self.margins)
            self._hyp[it] = (cnt, (it, R, t, mask, idx))
        return self._hyp[it]

    def refine(self, best):
        """Refine (:266-311): a pure function of the best set"""
        mask = best[3]
        key = mask.tobytes()
        if key not in self._ref:
            R, t = self._epnp(np.nonzero(mask)[0], True)
            rmask, cnt = check_inliers(R, t, self.corrs, self.cam, self.p["th2"], self.margins)
            self._ref[key] = (cnt > self.min_inliers, (R, t, rmask, cnt))
        return self._ref[key]

    def iterate(self, n, closed=None):
        """One call of iterate(n): dict(status, n_inliers, Tcw float32 4x4, Tcw_d, mask, at_iteration, iterations, hypotheses_run, refines_run)."""
        closed = (self.kind == "independent") if closed is None else closed
        it0 = self.state["iterations"]
        had = self.state["best"]
        r = (ransac_records if closed else ransac_literal)(self.state, n, self.N, self.min_inliers, self.max_its, self.hypothesis, self.refine)
        out = dict(status=r["status"], n_inliers=0, Tcw=np.zeros((4, 4), F32), Tcw_d=np.zeros((4, 4), F64), mask=None, at_iteration=r["at_iteration"],
                   iterations=self.state["iterations"], hypotheses_run=0, refines_run=0)
        if r["status"] == TOO_FEW:
            return out
        out["hypotheses_run"] = passes_of(it0, self.max_its, n)
        seen = []
        for b in r["refine_calls"]:                                # distinct best sets: what the device evaluates
            if not any(b is s for s in seen):
                seen.append(b)
        out["refines_run"] = len(seen)
        best = self.state["best"]
        if best is not None and best is not had:
            self.best_mask = best[3].copy()
            self.best_Tcw = pose4(best[1], best[2]).astype(F32)
        if r["status"] == REFINED:
            R, t, rmask, cnt = r["payload"]
            out.update(n_inliers=cnt, Tcw_d=pose4(R, t), mask=rmask.copy())
            out["Tcw"] = out["Tcw_d"].astype(F32)
        elif r["status"] == BEST:
            out.update(n_inliers=self.state["best_inliers"], mask=self.best_mask.copy(), Tcw=self.best_Tcw.copy())
            out["Tcw_d"] = pose4(best[1], best[2]) if best is not had else self.best_Tcw.astype(F64)
        if out["status"] in (REFINED, BEST) and not (np.all(np.isfinite(out["Tcw_d"])) and np.all(np.isfinite(out["Tcw"]))):
            out["status"] = NONFINITE
        return out
