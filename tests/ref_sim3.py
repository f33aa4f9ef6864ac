"""Reference for the batched Horn Sim3 RANSAC (Sim3Solver, src/estimators/Sim3Solver.cc), three times.

D19          what the library must EQUAL: one IEEE operation per numpy operation in the order DESIGN.md D19 states, np.float32 where the source
             narrows.  The operations are elementwise over the hypotheses of a call (axis 0) and over the correspondences: an elementwise numpy
             operation is the scalar operation on every element, so this is the scalar definition evaluated for many hypotheses at once.  Nothing
             is summed across an axis by numpy: every sum is written out term by term.
LITERAL      ComputeSim3 as the source writes step 4: the eigenvector of N (numpy.linalg.eigh on the float matrix widened), atan2 of the norm of
             its imaginary part and its real part, the angle-axis vector, the Rodrigues formula — all in double, narrowed once.  Everything else
             is D19's.  `literal_rotation` is what D19's R is held to within 2^-23 per entry.
INDEPENDENT  Umeyama's closed form in float64 by numpy.linalg.svd (`umeyama`): no quaternion, no eigenvector.

The RANSAC loop exists twice: `Solver.iterate_loop` is Sim3Solver::iterate as it is written, `closed_form` the walk over the count sequence that
the device runs; tests/test_sim3_ref.py holds one to the other exhaustively.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
EIG_SWEEPS = 10
DRAW_STRIDE = 4
TOO_FEW, FOUND, CONTINUE, EXHAUSTED, NONFINITE = 0, 1, 2, 3, 4
CORR_DTYPE = np.dtype([("X1c", "<f4", 3), ("sigma2_1", "<f4"), ("X2c", "<f4", 3), ("sigma2_2", "<f4"), ("idx1", "<i4"), ("_pad", "<i4", 3)])
DEFAULT = dict(probability=0.99, min_inliers=20, max_iterations=300, fix_scale=0, seed=0)      # LoopClosing.cc: SetRansacParameters(0.99, 20, 300)


def D(a):
    return np.asarray(a).astype(F64)


# ---------------------------------------------------------------- SetRansacParameters (:118-142)
def _log(x):
    """glibc's log with C's answers at the edges (math.log raises there)"""
    if x != x or x < 0:
        return float("nan")
    if x == 0:
        return float("-inf")
    return math.log(x) if x != float("inf") else x


def plan(N, probability=0.99, min_inliers=20, max_iterations=300, **_):
    """(max_iterations, epsilon as float32)"""
    with np.errstate(all="ignore"):
        eps = F32(min_inliers) / F32(N)
        if min_inliers == N:
            its = 1
        else:
            try:
                cube = math.pow(float(eps), 3)
            except OverflowError:
                cube = float("inf")
            x = np.ceil(F64(_log(1 - probability)) / F64(_log(1 - cube)))
            its = 2147483647 if x >= 2147483647.0 else int(x) if x >= 1.0 else 1      # a NaN or a non-positive count ends as 1
    return max(1, min(its, max_iterations)), eps


# ---------------------------------------------------------------- the draws (DESIGN.md D18 with a set of 3)
_M64 = (1 << 64) - 1


def mix(c):
    z = (0x9E3779B97F4A7C15 * ((c + 1) & _M64)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def draw32(seed, it, k, draws=None):
    if draws is not None and it < len(draws):
        return int(draws[it][k])
    return mix((seed + 3 * it + k) & _M64) >> 32


def sample(N, words):
    """:167-181 on a Python list: idx = avail[randi]; avail[idx] = avail.back(); pop.  The write goes to the place named by the VALUE.  A std::vector
    keeps its storage after a pop, so a write to a popped place touches memory nobody reads again: here it is skipped."""
    avail = list(range(N))
    out = []
    for k in range(3):
        randi = (int(words[k]) * len(avail)) >> 32
        idx = avail[randi]
        out.append(idx)
        if idx < len(avail):
            avail[idx] = avail[-1]
        avail.pop()
    return out


# ---------------------------------------------------------------- thresholds, projections, CheckInliers
def threshold(sigma2):
    """mvnMaxError: size_t(9.210 * sigma2) as a float; 0 where the conversion is undefined"""
    s = np.atleast_1d(np.asarray(sigma2, F32))
    with np.errstate(all="ignore"):
        d = F64(9.210) * D(s)
        ok = (d >= 0) & (d < 18446744073709551616.0)
    out = np.zeros(s.shape, F32)
    out[ok] = d[ok].astype(np.uint64).astype(F32)
    return out


def image(X, k):
    """FromCameraToImage: X [..., 3] float32, k = (fx, fy, cx, cy) float32"""
    with np.errstate(all="ignore"):
        invz = F32(1) / X[..., 2]
        x, y = X[..., 0] * invz, X[..., 1] * invz
        return np.stack([k[0] * x + k[2], k[1] * y + k[3]], -1)


def project(T, X, k):
    """Project: T [H, 3, 4] float32, X [N, 3] float32 -> [H, N, 2]"""
    with np.errstate(all="ignore"):
        P = [((((D(T[:, i, 0])[:, None] * D(X[:, 0])[None] + D(T[:, i, 1])[:, None] * D(X[:, 1])[None]) + D(T[:, i, 2])[:, None] * D(X[:, 2])[None])
              + D(T[:, i, 3])[:, None]).astype(F32)) for i in range(3)]
        return image(np.stack(P, -1), k)


def errors(a, b, corrs, k1, k2):
    """err1, err2 [H, N] float32 of CheckInliers for the transforms a (T12) and b (T21)"""
    p1, p2 = image(corrs["X1c"], k1), image(corrs["X2c"], k2)
    with np.errstate(all="ignore"):
        d1 = p1[None] - project(a, corrs["X2c"], k1)
        d2 = project(b, corrs["X1c"], k2) - p2[None]
        e1 = (D(d1[..., 0]) * D(d1[..., 0]) + D(d1[..., 1]) * D(d1[..., 1])).astype(F32)
        e2 = (D(d2[..., 0]) * D(d2[..., 0]) + D(d2[..., 1]) * D(d2[..., 1])).astype(F32)
    return e1, e2


def errors64(a, b, corrs, k1, k2):
    """the same two errors in float64 throughout, at the same (float) transforms: what the float pipeline's rounding is measured against"""
    def img(X, k):
        return np.stack([D(k[0]) * (X[..., 0] / X[..., 2]) + D(k[2]), D(k[1]) * (X[..., 1] / X[..., 2]) + D(k[3])], -1)
    with np.errstate(all="ignore"):
        a, b, X1, X2 = D(a), D(b), D(corrs["X1c"]), D(corrs["X2c"])
        d1 = img(X1, k1)[None] - img(np.einsum("hij,nj->hni", a[:, :, :3], X2) + a[:, None, :, 3], k1)
        d2 = img(np.einsum("hij,nj->hni", b[:, :, :3], X1) + b[:, None, :, 3], k2) - img(X2, k2)[None]
        return (d1 * d1).sum(-1), (d2 * d2).sum(-1)


def inliers(a, b, corrs, k1, k2):
    e1, e2 = errors(a, b, corrs, k1, k2)
    with np.errstate(all="ignore"):
        return (e1 < threshold(corrs["sigma2_1"])[None]) & (e2 < threshold(corrs["sigma2_2"])[None])


# ---------------------------------------------------------------- ComputeSim3 (:230-341) under D19
def _rotate(A, V, p, q):
    with np.errstate(all="ignore"):
        apq = A[:, p, q].copy()
        do = np.abs(apq) > 0
        theta = (A[:, q, q] - A[:, p, p]) / (F64(2) * apq)
        t = np.where(theta < 0, F64(-1), F64(1)) / (np.abs(theta) + np.sqrt(theta * theta + F64(1)))
        c = F64(1) / np.sqrt(t * t + F64(1))
        s = t * c
        for k in range(4):
            x, y = A[:, k, p].copy(), A[:, k, q].copy()
            A[:, k, p], A[:, k, q] = np.where(do, c * x - s * y, x), np.where(do, s * x + c * y, y)
        for k in range(4):
            x, y = A[:, p, k].copy(), A[:, q, k].copy()
            A[:, p, k], A[:, q, k] = np.where(do, c * x - s * y, x), np.where(do, s * x + c * y, y)
        for k in range(4):
            x, y = V[:, k, p].copy(), V[:, k, q].copy()
            V[:, k, p], V[:, k, q] = np.where(do, c * x - s * y, x), np.where(do, s * x + c * y, y)


def horn_matrix(x1, x2):
    """steps 1 to 3: (O1, O2, Pr1, Pr2 [H, r, k] float32, N [H, 4, 4] float32)"""
    x1, x2 = np.asarray(x1, F32), np.asarray(x2, F32)             # [H, k, r]
    with np.errstate(all="ignore"):
        O1 = ((x1[:, 0] + x1[:, 1]) + x1[:, 2]) / F32(3)
        O2 = ((x2[:, 0] + x2[:, 1]) + x2[:, 2]) / F32(3)
        Pr1 = x1.transpose(0, 2, 1) - O1[:, :, None]
        Pr2 = x2.transpose(0, 2, 1) - O2[:, :, None]
        m = np.zeros((len(x1), 3, 3), F64)
        for i in range(3):
            for j in range(3):
                m[:, i, j] = D(((D(Pr2[:, i, 0]) * D(Pr1[:, j, 0]) + D(Pr2[:, i, 1]) * D(Pr1[:, j, 1])) + D(Pr2[:, i, 2]) * D(Pr1[:, j, 2])).astype(F32))
        N11, N12, N13, N14 = m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2], m[:, 1, 2] - m[:, 2, 1], m[:, 2, 0] - m[:, 0, 2], m[:, 0, 1] - m[:, 1, 0]
        N22, N23, N24 = m[:, 0, 0] - m[:, 1, 1] - m[:, 2, 2], m[:, 0, 1] + m[:, 1, 0], m[:, 2, 0] + m[:, 0, 2]
        N33, N34, N44 = -m[:, 0, 0] + m[:, 1, 1] - m[:, 2, 2], m[:, 1, 2] + m[:, 2, 1], -m[:, 0, 0] - m[:, 1, 1] + m[:, 2, 2]
    N = np.stack([np.stack(r, -1) for r in ((N11, N12, N13, N14), (N12, N22, N23, N24), (N13, N23, N33, N34), (N14, N24, N34, N44))], 1).astype(F32)
    return O1, O2, Pr1, Pr2, N


def jacobi_quaternion(N):
    """the eigenvector of the largest eigenvalue of N [H, 4, 4] by the cyclic Jacobi of D19, w >= 0: [H, 4] float64"""
    A = D(N).copy()
    V = np.tile(np.eye(4, dtype=F64), (len(A), 1, 1))
    for _ in range(EIG_SWEEPS):
        for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            _rotate(A, V, p, q)
    lam, quat = A[:, 0, 0].copy(), V[:, :, 0].copy()
    for j in range(1, 4):
        with np.errstate(all="ignore"):
            g = A[:, j, j] > lam
        lam = np.where(g, A[:, j, j], lam)
        quat = np.where(g[:, None], V[:, :, j], quat)
    return np.where((quat[:, 0] < 0)[:, None], -quat, quat)


def quaternion_rotation(quat):
    """D19's R [H, 3, 3] float64 from the quaternion; non-finite for a zero imaginary part, as :284 divides 0 by 0"""
    w, x, y, z = quat[:, 0], quat[:, 1], quat[:, 2], quat[:, 3]
    with np.errstate(all="ignore"):
        ww, xx, yy, zz, xy, xz, yz, wx, wy, wz = w * w, x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
        n = ((ww + xx) + yy) + zz
        two = F64(2)
        R = np.stack([(((ww + xx) - yy) - zz) / n, (two * (xy - wz)) / n, (two * (xz + wy)) / n,
                      (two * (xy + wz)) / n, (((ww - xx) + yy) - zz) / n, (two * (yz - wx)) / n,
                      (two * (xz - wy)) / n, (two * (yz + wx)) / n, (((ww - xx) - yy) + zz) / n], -1)
    R[(x == 0) & (y == 0) & (z == 0)] = np.nan
    return R.reshape(-1, 3, 3)


def literal_rotation(N):
    """step 4 as the source writes it, in double: eigenvector (numpy.linalg.eigh), atan2, angle-axis, Rodrigues.  [H, 3, 3] float64"""
    out = np.zeros((len(N), 3, 3), F64)
    for h, n in enumerate(D(N)):
        if not np.isfinite(n).all():
            out[h] = np.nan
            continue
        val, vec = np.linalg.eigh(n)
        q = vec[:, int(np.argmax(val))]
        v = q[1:4].copy()
        with np.errstate(all="ignore"):
            nrm = math.sqrt(float(v @ v))
            ang = math.atan2(nrm, q[0])
            rv = 2 * ang * v / F64(nrm)                            # 0 / 0 for a zero imaginary part
            th = math.sqrt(float(rv @ rv)) if np.isfinite(rv).all() else float("nan")
            if not th == th:
                out[h] = np.nan
                continue
            r = rv / th
            c, s = math.cos(th), math.sin(th)
            K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
            out[h] = c * np.eye(3) + (1 - c) * np.outer(r, r) + s * K
    return out


def finish_pose(R64, O1, O2, Pr1, Pr2, fix_scale):
    """steps 5 to 7 from a double R: (R float32 [H, 3, 3], t [H, 3], s [H])"""
    R = R64.astype(F32)
    H = len(R)
    with np.errstate(all="ignore"):
        if fix_scale:
            s = np.ones(H, F32)
        else:
            nom, den = np.zeros(H, F64), np.zeros(H, F64)
            for i in range(3):
                for k in range(3):
                    p3 = ((D(R[:, i, 0]) * D(Pr2[:, 0, k]) + D(R[:, i, 1]) * D(Pr2[:, 1, k])) + D(R[:, i, 2]) * D(Pr2[:, 2, k])).astype(F32)
                    nom = nom + D(Pr1[:, i, k]) * D(p3)
                    den = den + D(p3 * p3)
            s = (nom / den).astype(F32)
        t = np.stack([(D(O1[:, i]) - D(s) * ((D(R[:, i, 0]) * D(O2[:, 0]) + D(R[:, i, 1]) * D(O2[:, 1])) + D(R[:, i, 2]) * D(O2[:, 2]))).astype(F32)
                      for i in range(3)], -1)
    return R, t, s


def transforms(R, t, s):
    """steps 8.1 and 8.2: the upper three rows of T12 and T21, [H, 3, 4] float32 each"""
    H = len(R)
    a, b = np.zeros((H, 3, 4), F32), np.zeros((H, 3, 4), F32)
    with np.errstate(all="ignore"):
        alpha = F64(1) / D(s)
        a[:, :, :3] = s[:, None, None] * R
        a[:, :, 3] = t
        for i in range(3):
            for j in range(3):
                b[:, i, j] = (alpha * D(R[:, j, i])).astype(F32)
        for i in range(3):
            b[:, i, 3] = (-((D(b[:, i, 0]) * D(t[:, 0]) + D(b[:, i, 1]) * D(t[:, 1])) + D(b[:, i, 2]) * D(t[:, 2]))).astype(F32)
    return a, b


def solve(x1, x2, fix_scale, rotation="d19"):
    """ComputeSim3 for H samples x[h][k][r]: (R, t, s, a, b)"""
    O1, O2, Pr1, Pr2, N = horn_matrix(x1, x2)
    R64 = quaternion_rotation(jacobi_quaternion(N)) if rotation == "d19" else literal_rotation(N)
    R, t, s = finish_pose(R64, O1, O2, Pr1, Pr2, fix_scale)
    return (R, t, s) + transforms(R, t, s)


def umeyama(x1, x2, fix_scale):
    """INDEPENDENT: s, R, t with x1 ~ s R x2 + t for one sample x[k][r], float64, by SVD"""
    A, B = D(x1), D(x2)
    ma, mb = A.mean(0), B.mean(0)
    Ac, Bc = A - ma, B - mb
    U, S, Vt = np.linalg.svd(Ac.T @ Bc)
    d = np.sign(np.linalg.det(U @ Vt))
    R = U @ np.diag([1, 1, d]) @ Vt
    RB = Bc @ R.T
    s = 1.0 if fix_scale else float((Ac * RB).sum() / (RB * RB).sum())
    return s, R, ma - s * R @ mb


def T44(a):
    out = np.zeros(16, F32)
    out[:12], out[15] = np.asarray(a, F32).reshape(-1), 1
    return out


# ---------------------------------------------------------------- the solver
class Solver:
    """one problem: corrs (CORR_DTYPE), cameras k1, k2 = (fx, fy, cx, cy), params as DEFAULT, draws uint32 [cap, DRAW_STRIDE] or None"""

    def __init__(self, corrs, k1, k2, params=None, draws=None, rotation="d19"):
        self.corrs = np.ascontiguousarray(corrs, CORR_DTYPE).reshape(-1)
        self.k1, self.k2 = np.asarray(k1, F32), np.asarray(k2, F32)
        self.params = dict(DEFAULT, **(params or {}))
        self.draws, self.rotation = draws, rotation
        self.N = len(self.corrs)
        self.max_its, self.epsilon = plan(self.N, **self.params)
        self.min_inliers = self.params["min_inliers"]
        self.iterations, self.best_inliers = 0, 0
        self.best = None                                           # (R, t, s, T12 [16])
        self.best_mask = np.zeros(self.N, np.uint8)

    def hypotheses(self, it0, n):
        """iterations it0 .. it0+n-1: (samples [n][3], R, t, s, a, b, masks [n, N])"""
        smp = [sample(self.N, [draw32(self.params["seed"], it, k, self.draws) for k in range(3)]) for it in range(it0, it0 + n)]
        idx = np.array(smp, np.int64).reshape(n, 3)
        R, t, s, a, b = solve(self.corrs["X1c"][idx], self.corrs["X2c"][idx], self.params["fix_scale"], self.rotation)
        return smp, R, t, s, a, b, inliers(a, b, self.corrs, self.k1, self.k2)

    def passes(self, n):
        return max(0, min(self.max_its - self.iterations, n))

    def _result(self, status, hyps, found=None):
        r = dict(status=status, n_inliers=0, at_iteration=0, iterations=self.iterations, hypotheses_run=hyps, T12=np.zeros(16, F32), R=np.zeros(9, F32),
                 t=np.zeros(3, F32), s=F32(0), mask=np.zeros(self.N, np.uint8))
        if found is not None:
            R, t, s, T12 = self.best
            ok = np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(s) and np.isfinite(T12).all()
            r.update(status=FOUND if ok else NONFINITE, n_inliers=self.best_inliers, at_iteration=self.iterations, T12=T12, R=R.reshape(-1), t=t, s=s,
                     mask=self.best_mask.copy())
        return r

    def iterate_loop(self, n):
        """Sim3Solver::iterate as it is written (:144-211)"""
        if self.N < self.min_inliers or self.N < 3:
            return self._result(TOO_FEW, 0)
        n_run = self.passes(n)
        if n_run:
            _, R, t, s, a, b, masks = self.hypotheses(self.iterations, n_run)
        cur = 0
        while self.iterations < self.max_its and cur < n:
            j = cur
            cur += 1
            self.iterations += 1
            cnt = int(masks[j].sum())
            if cnt >= self.best_inliers:
                self.best_mask, self.best_inliers = masks[j].astype(np.uint8), cnt
                self.best = (R[j].copy(), t[j].copy(), s[j], T44(a[j]))
                if cnt > self.min_inliers:
                    return self._result(FOUND, n_run, found=j)
        return self._result(EXHAUSTED if self.iterations >= self.max_its else CONTINUE, n_run)

    def iterate(self, n):
        """the same call through the closed form over the counts"""
        if self.N < self.min_inliers or self.N < 3:
            return self._result(TOO_FEW, 0)
        n_run = self.passes(n)
        found = rec = None
        if n_run:
            _, R, t, s, a, b, masks = self.hypotheses(self.iterations, n_run)
            found, rec, best = closed_form([int(m.sum()) for m in masks], self.best_inliers, self.min_inliers)
        if rec is not None:
            self.best_mask, self.best_inliers = masks[rec].astype(np.uint8), best
            self.best = (R[rec].copy(), t[rec].copy(), s[rec], T44(a[rec]))
        self.iterations += n_run if found is None else found + 1
        if found is not None:
            return self._result(FOUND, n_run, found=found)
        return self._result(EXHAUSTED if self.iterations >= self.max_its else CONTINUE, n_run)

    def find(self):
        return self.iterate(self.max_its)


def closed_form(counts, best0, min_inliers):
    """(found, rec, best): the walk returns at the first j with c_j >= max(best0, c_0 .. c_{j-1}) and c_j > min_inliers; otherwise the best is the LAST
    index attaining the prefix maximum, provided that maximum is >= best0 (rec None: the state's best stands)"""
    c = list(counts)
    for j in range(len(c)):
        if c[j] >= max([best0] + c[:j]) and c[j] > min_inliers:
            return j, j, c[j]
    if not c or max(c) < best0:
        return None, None, best0
    top = max(c)
    return None, max(j for j in range(len(c)) if c[j] == top), top


def loop_form(counts, best0, min_inliers):
    """the loop of :162-205 over a count sequence, as it is written"""
    best, rec = best0, None
    for j, cnt in enumerate(counts):
        if cnt >= best:
            best, rec = cnt, j
            if cnt > min_inliers:
                return j, rec, best
    return None, rec, best
