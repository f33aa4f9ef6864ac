"""Optimizer::PoseOptimization (src/optimizers/Optimizer.cc:48-279) with the parts of g2o it runs through, restated from the reference's text in
float64, twice:

  pose_optimization_literal   edge by edge in g2o's order, a Quat / SE3 class after g2o's SE3Quat, Python floats (IEEE double, no contraction)
  pose_optimization_fast      the same statements on numpy arrays; every accumulation is np.add.accumulate, which adds strictly left to right, so
                              the two versions agree bit for bit (tests/test_poseopt_ref.py pins that)

Both take `sum_order`: a permutation of the edges in which every accumulation (chi sums, H, b) visits the active edges.  None is g2o's order
(ascending edge index).  The spread of the result over a few seeded permutations is the reference's own sensitivity to the order of summation.

A problem is (Tcw float32 4x4, cam = (fx, fy, cx, cy, bf) float32, edges) with edges a numpy array of EDGE_DTYPE = hs_pose_edge.  The result is a
dict: Tcw_d (4, 4) float64, Tcw float32, outlier uint8 [n], n_edges, n_good, rounds, lm_iterations, lm_trials, status, and for the tests
round_flags (rounds, n), min_margin (the smallest |chi2/th - 1| over every classification), max_trials (the most trials of one iteration) and
empty_rounds.  DESIGN.md section 5.11 lists the behaviour item by item; D13 and D14 state what is restated from knowledge (Eigen is not in the
reference tree) and the stale-error rule."""
import math

import numpy as np

EDGE_DTYPE = np.dtype([("Xw", "<f4", 3), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("inv_sigma2", "<f4"), ("kp", "<i4")])
F32 = np.float32
TH_MONO, TH_STEREO = F32(5.991), F32(7.815)                      # const float chi2Mono[4], chi2Stereo[4]
DELTA_MONO, DELTA_STEREO = float(F32(math.sqrt(5.991))), float(F32(math.sqrt(7.815)))   # const float deltaMono = sqrt(5.991)
STATUS_OK, STATUS_TOO_FEW, STATUS_NONFINITE = 0, 1, 2
DBL_MAX = float(np.finfo(np.float64).max)


def inv_sigma2(size, size_ref=31.0, sigma_ref=1.0):
    """1 / determineSigma2(size) in float (FeatureExtractorSettings.cpp:5-8, Optimizer.cc:124)"""
    with np.errstate(all="ignore"):
        s = F32(size) / F32(size_ref)
        return F32(1.0) / (F32(sigma_ref) * (s * s))


# ---------------------------------------------------------------- SE3Quat (se3quat.h) with Eigen's Quaterniond restated
class Quat:
    __slots__ = ("x", "y", "z", "w")

    def __init__(self, w, x, y, z):
        self.w, self.x, self.y, self.z = w, x, y, z

    @staticmethod
    def from_matrix(m):                                          # Quaterniond(Matrix3d)
        t = m[0][0] + m[1][1] + m[2][2]
        if t > 0.0:
            t = math.sqrt(t + 1.0)
            w = 0.5 * t
            t = 0.5 / t
            return Quat(w, (m[2][1] - m[1][2]) * t, (m[0][2] - m[2][0]) * t, (m[1][0] - m[0][1]) * t)
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        v = [0.0, 0.0, 0.0]
        v[i] = 0.5 * t
        t = 0.5 / t
        w = (m[k][j] - m[j][k]) * t
        v[j] = (m[j][i] + m[i][j]) * t
        v[k] = (m[k][i] + m[i][k]) * t
        return Quat(w, v[0], v[1], v[2])

    def matrix(self):                                            # toRotationMatrix()
        tx, ty, tz = 2.0 * self.x, 2.0 * self.y, 2.0 * self.z
        twx, twy, twz = tx * self.w, ty * self.w, tz * self.w
        txx, txy, txz = tx * self.x, ty * self.x, tz * self.x
        tyy, tyz, tzz = ty * self.y, tz * self.y, tz * self.z
        return [[1.0 - (tyy + tzz), txy - twz, txz + twy],
                [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]

    def mul(self, b):                                            # a * b
        a = self
        return Quat(a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z,
                    a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
                    a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
                    a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x)

    def rotate(self, v):                                         # q * v: v + w * uv + q.vec x uv with uv = 2 (q.vec x v)
        ux = self.y * v[2] - self.z * v[1]
        uy = self.z * v[0] - self.x * v[2]
        uz = self.x * v[1] - self.y * v[0]
        ux, uy, uz = ux + ux, uy + uy, uz + uz
        return [v[0] + self.w * ux + (self.y * uz - self.z * uy),
                v[1] + self.w * uy + (self.z * ux - self.x * uz),
                v[2] + self.w * uz + (self.x * uy - self.y * ux)]

    def normalized(self):                                        # normalizeRotation(): w >= 0, then normalize()
        x, y, z, w = self.x, self.y, self.z, self.w
        if w < 0:
            x, y, z, w = -x, -y, -z, -w
        n = math.sqrt(x * x + y * y + z * z + w * w)
        return Quat(w / n, x / n, y / n, z / n)


class SE3:
    __slots__ = ("r", "t")

    def __init__(self, r, t):
        self.r, self.t = r.normalized(), list(t)

    def mul(self, b):                                            # operator*: _t += _r * b._t; _r *= b._r; normalizeRotation()
        rt = self.r.rotate(b.t)
        return SE3(self.r.mul(b.r), [self.t[0] + rt[0], self.t[1] + rt[1], self.t[2] + rt[2]])

    def map(self, v):                                            # _r * xyz + _t
        p = self.r.rotate(v)
        return [p[0] + self.t[0], p[1] + self.t[1], p[2] + self.t[2]]

    def matrix(self):                                            # to_homogeneous_matrix()
        m = np.eye(4)
        m[:3, :3] = self.r.matrix()
        m[:3, 3] = self.t
        return m

    def key(self):
        return (self.r.w, self.r.x, self.r.y, self.r.z) + tuple(self.t)


def se3_from_pose(Tcw):                                          # Converter::toSE3Quat: floats widened, SE3Quat(R, t)
    T = np.asarray(Tcw, np.float32).reshape(4, 4).astype(np.float64)
    return SE3(Quat.from_matrix([[float(T[i, j]) for j in range(3)] for i in range(3)]), [float(T[i, 3]) for i in range(3)])


def se3_exp(u):                                                  # SE3Quat::exp(update): omega = u[0:3], upsilon = u[3:6]
    ox, oy, oz = u[0], u[1], u[2]
    theta = math.sqrt(ox * ox + oy * oy + oz * oz)
    Om = [[0.0, -oz, oy], [oz, 0.0, -ox], [-oy, ox, 0.0]]
    Om2 = [[(Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j]) + Om[i][2] * Om[2][j] for j in range(3)] for i in range(3)]
    if theta < 0.00001:
        a, b, c, d = 1.0, 0.5, 0.5, 1.0 / 6.0
    else:
        a = math.sin(theta) / theta
        b = (1.0 - math.cos(theta)) / (theta * theta)
        c = b
        d = (theta - math.sin(theta)) / (theta * theta * theta)
    eye = lambda i, j: 1.0 if i == j else 0.0
    R = [[(eye(i, j) + a * Om[i][j]) + b * Om2[i][j] for j in range(3)] for i in range(3)]
    V = [[(eye(i, j) + c * Om[i][j]) + d * Om2[i][j] for j in range(3)] for i in range(3)]
    t = [(V[i][0] * u[3] + V[i][1] * u[4]) + V[i][2] * u[5] for i in range(3)]
    return SE3(Quat.from_matrix(R), t)


def ldlt_solve(H, lam, b):
    """(H + lam I) x = b by LDL^T without pivoting; None where a pivot is not positive (`_cholesky.info() != Eigen::Success`, D13)"""
    A = [[H[i][j] for j in range(6)] for i in range(6)]
    for i in range(6):
        A[i][i] = A[i][i] + lam
    L = [[0.0] * 6 for _ in range(6)]
    d = [0.0] * 6
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s = s - (L[j][k] * L[j][k]) * d[k]
        if s <= 0.0:
            return None
        d[j] = s
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s = s - (L[i][k] * L[j][k]) * d[k]
            L[i][j] = s / d[j]
    y = [0.0] * 6
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s
    for i in range(6):
        y[i] = y[i] / d[i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s
    return x


def huber(e, delta):                                             # RobustKernelHuber::robustify: (rho[0], rho[1])
    dsqr = delta * delta
    if e <= dsqr:
        return e, 1.0
    sq = math.sqrt(e)
    return 2 * sq * delta - dsqr, delta / sq


# ---------------------------------------------------------------- the per-edge statements, literal
def _fdiv(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return float("nan")
        return math.copysign(float("inf"), a) * math.copysign(1.0, b)


def edge_error(T, X, obs, cam, stereo):
    """computeError(): obs - cam_project(estimate.map(Xw)) (types_six_dof_expmap.h:242-246,303-307; .cpp:571-586)"""
    fx, fy, cx, cy, bf = cam
    p = T.map(X)
    if not stereo:
        return [obs[0] - (_fdiv(p[0], p[2]) * fx + cx), obs[1] - (_fdiv(p[1], p[2]) * fy + cy)]
    with np.errstate(all="ignore"):
        invz = float(F32(_fdiv(1.0, p[2])))                      # const float invz = 1.0f / trans_xyz[2]: a double quotient narrowed to float
    r0 = p[0] * invz * fx + cx
    return [obs[0] - r0, obs[1] - (p[1] * invz * fy + cy), obs[2] - (r0 - bf * invz)]


def edge_jacobian(T, X, cam, stereo):
    """linearizeOplus() (types_six_dof_expmap.cpp:547-569,614-643): rows of 6"""
    fx, fy, _, _, bf = cam
    x, y, z = T.map(X)
    invz = _fdiv(1.0, z)
    invz_2 = invz * invz
    J = [[x * y * invz_2 * fx, -(1 + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, 0.0, x * invz_2 * fx],
         [(1 + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, 0.0, -invz * fy, y * invz_2 * fy]]
    if stereo:
        J.append([J[0][0] - bf * y * invz_2, J[0][1] + bf * x * invz_2, J[0][2], J[0][3], 0.0, J[0][5] - bf * invz_2])
    return J


def chi2_of(e, w):                                               # _error.dot(information() * _error)
    s = e[0] * (w * e[0])
    for k in range(1, len(e)):
        s = s + e[k] * (w * e[k])
    return s


class _Literal:
    def __init__(self, cam, edges):
        self.cam = [float(c) for c in cam]
        self.n = len(edges)
        self.X = [[float(v) for v in e["Xw"]] for e in edges]
        self.stereo = [not (float(e["ur"]) < 0) for e in edges]  # if(views.uR(i)<0) mono else stereo
        self.obs = [[float(e["u"]), float(e["v"]), float(e["ur"])] for e in edges]
        self.w = [float(e["inv_sigma2"]) for e in edges]

    def chi2(self, T, i):
        return chi2_of(edge_error(T, self.X[i], self.obs[i], self.cam, self.stereo[i]), self.w[i])

    def chi2_all(self, T):
        return np.array([self.chi2(T, i) for i in range(self.n)], np.float64)

    def robust_chi(self, T, order, robust):                      # computeActiveErrors(); activeRobustChi2()
        chi = 0.0
        for i in order:
            c = self.chi2(T, i)
            chi = chi + (huber(c, DELTA_STEREO if self.stereo[i] else DELTA_MONO)[0] if robust else c)
        return chi

    def system(self, T, order, robust):                          # computeActiveErrors(); activeRobustChi2(); buildSystem()
        H = [[0.0] * 6 for _ in range(6)]
        b = [0.0] * 6
        chi = 0.0
        for i in order:
            e = edge_error(T, self.X[i], self.obs[i], self.cam, self.stereo[i])
            w = self.w[i]
            c = chi2_of(e, w)
            r0, r1 = huber(c, DELTA_STEREO if self.stereo[i] else DELTA_MONO) if robust else (c, 1.0)
            chi = chi + r0
            J = edge_jacobian(T, self.X[i], self.cam, self.stereo[i])
            D = len(J)
            for a in range(6):
                # b -= rho[1] * A^T * omega * e;  H += A^T * (rho[1] * omega) * A   (base_unary_edge.hpp:62-73; no rho[1] without a kernel)
                if robust:
                    s = ((r1 * J[0][a]) * w) * e[0]
                    for k in range(1, D):
                        s = s + ((r1 * J[k][a]) * w) * e[k]
                else:
                    s = (J[0][a] * w) * e[0]
                    for k in range(1, D):
                        s = s + (J[k][a] * w) * e[k]
                b[a] = b[a] - s
                ww = r1 * w if robust else w
                for c2 in range(a, 6):
                    s = (J[0][a] * ww) * J[0][c2]
                    for k in range(1, D):
                        s = s + (J[k][a] * ww) * J[k][c2]
                    H[a][c2] = H[a][c2] + s
        for a in range(6):
            for c2 in range(a):
                H[a][c2] = H[c2][a]
        return H, b, chi


# ---------------------------------------------------------------- the same statements on arrays
class _Fast:
    def __init__(self, cam, edges):
        self.cam = [float(c) for c in cam]
        self.n = len(edges)
        self.X = edges["Xw"].astype(np.float64).reshape(-1, 3)
        self.u, self.v, self.ur = (edges[k].astype(np.float64) for k in ("u", "v", "ur"))
        self.stereo = ~(edges["ur"] < 0)
        self.w = edges["inv_sigma2"].astype(np.float64)
        self.delta = np.where(self.stereo, DELTA_STEREO, DELTA_MONO)

    def _map(self, T, idx):
        q, t, X = T.r, T.t, self.X[idx]
        ux = q.y * X[:, 2] - q.z * X[:, 1]
        uy = q.z * X[:, 0] - q.x * X[:, 2]
        uz = q.x * X[:, 1] - q.y * X[:, 0]
        ux, uy, uz = ux + ux, uy + uy, uz + uz
        return (X[:, 0] + q.w * ux + (q.y * uz - q.z * uy) + t[0], X[:, 1] + q.w * uy + (q.z * ux - q.x * uz) + t[1],
                X[:, 2] + q.w * uz + (q.x * uy - q.y * ux) + t[2])

    def _errors(self, T, idx):
        fx, fy, cx, cy, bf = self.cam
        x, y, z = self._map(T, idx)
        st = self.stereo[idx]
        with np.errstate(all="ignore"):
            invz = (1.0 / z).astype(np.float32).astype(np.float64)
            r0 = np.where(st, x * invz * fx + cx, (x / z) * fx + cx)
            r1 = np.where(st, y * invz * fy + cy, (y / z) * fy + cy)
            e0, e1, e2 = self.u[idx] - r0, self.v[idx] - r1, self.ur[idx] - (r0 - bf * invz)
            w = self.w[idx]
            c = e0 * (w * e0) + e1 * (w * e1)
            c = np.where(st, c + e2 * (w * e2), c)
        return (x, y, z), (e0, e1, e2), c

    def _huber(self, c, idx):
        d = self.delta[idx]
        dsqr = d * d
        with np.errstate(all="ignore"):
            sq = np.sqrt(c)
            inl = c <= dsqr
            return np.where(inl, c, 2 * sq * d - dsqr), np.where(inl, 1.0, d / sq)

    def chi2_all(self, T):
        return self._errors(T, np.arange(self.n))[2]

    @staticmethod
    def _sum(a):                                                 # strictly left to right, from 0
        return float(np.add.accumulate(a)[-1]) if len(a) else 0.0

    def robust_chi(self, T, order, robust):
        idx = np.asarray(order, np.int64)
        c = self._errors(T, idx)[2]
        return self._sum(self._huber(c, idx)[0] if robust else c)

    def system(self, T, order, robust):
        idx = np.asarray(order, np.int64)
        fx, fy, _, _, bf = self.cam
        (x, y, z), e, c = self._errors(T, idx)
        st, w = self.stereo[idx], self.w[idx]
        r0, r1 = self._huber(c, idx) if robust else (c, None)
        with np.errstate(all="ignore"):
            invz = 1.0 / z
            invz_2 = invz * invz
            zero = np.zeros_like(x)
            J0 = [x * y * invz_2 * fx, -(1 + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, zero, x * invz_2 * fx]
            J1 = [(1 + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, zero, -invz * fy, y * invz_2 * fy]
            J2 = [J0[0] - bf * y * invz_2, J0[1] + bf * x * invz_2, J0[2], J0[3], zero, J0[5] - bf * invz_2]
            H = [[0.0] * 6 for _ in range(6)]
            b = [0.0] * 6
            ww = r1 * w if robust else w
            for a in range(6):
                if robust:
                    s2 = ((r1 * J0[a]) * w) * e[0] + ((r1 * J1[a]) * w) * e[1]
                    s3 = s2 + ((r1 * J2[a]) * w) * e[2]
                else:
                    s2 = (J0[a] * w) * e[0] + (J1[a] * w) * e[1]
                    s3 = s2 + (J2[a] * w) * e[2]
                b[a] = self._sum(-np.where(st, s3, s2))
                for c2 in range(a, 6):
                    s2 = (J0[a] * ww) * J0[c2] + (J1[a] * ww) * J1[c2]
                    s3 = s2 + (J2[a] * ww) * J2[c2]
                    H[a][c2] = self._sum(np.where(st, s3, s2))
                    H[c2][a] = H[a][c2]
        return H, b, self._sum(r0)


# ---------------------------------------------------------------- Optimizer::PoseOptimization over either evaluator
def _finite(x):
    return not (math.isinf(x) or math.isnan(x))


def _levenberg(ev, T, order, robust, st):
    """SparseOptimizer::optimize(10) with OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:57-148).  Returns the
    estimate and the estimate the edges' errors belong to (D14)."""
    lam, ni = 0.0, 2.0
    dx = [0.0] * 6
    T_err = T
    for it in range(10):
        H, b, current = ev.system(T, order, robust)
        T_err = T
        st["lm_iterations"] += 1
        if it == 0:
            maxd = 0.0
            for j in range(6):
                a = abs(H[j][j])
                maxd = maxd if a < maxd else a                   # std::max(fabs(h), maxDiagonal)
            lam, ni = 1e-5 * maxd, 2.0
        rho, qmax = 0.0, 0
        while True:
            st["lm_trials"] += 1
            x = ldlt_solve(H, lam, b)
            ok2 = x is not None
            if ok2:
                dx = x
            backup = T                                           # push()
            T = se3_exp(dx).mul(T)                               # oplusImpl: setEstimate(SE3Quat::exp(update) * estimate())
            temp = ev.robust_chi(T, order, robust)
            T_err = T
            if not ok2:
                temp = DBL_MAX
            scale = 0.0
            for j in range(6):
                scale = scale + dx[j] * (lam * dx[j] + b[j])
            scale = scale + 1e-3
            with np.errstate(all="ignore"):
                rho = float(np.float64(current - temp) / np.float64(scale))
            if rho > 0 and _finite(temp):
                try:
                    alpha = 1.0 - (2 * rho - 1) ** 3             # 1.-pow((2*rho-1),3)
                except OverflowError:
                    alpha = -math.inf
                alpha = 2.0 / 3.0 if 2.0 / 3.0 < alpha else alpha
                lam = lam * (alpha if 1.0 / 3.0 < alpha else 1.0 / 3.0)
                ni = 2.0
                current = temp
            else:
                lam = lam * ni
                ni = ni * 2
                T = backup                                       # pop()
                if not _finite(lam):
                    break
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        st["max_trials"] = max(st["max_trials"], qmax)
        if qmax == 10 or rho == 0 or not _finite(lam):
            break                                                # Terminate
    return T, T_err


def _pose_optimization(make, Tcw, cam, edges, sum_order):
    edges = np.ascontiguousarray(edges, EDGE_DTYPE)
    n = len(edges)
    Tin = np.asarray(Tcw, np.float32).reshape(4, 4)
    out = dict(n_edges=n, n_good=0, rounds=0, lm_iterations=0, lm_trials=0, status=STATUS_TOO_FEW, Tcw_d=Tin.astype(np.float64), Tcw=Tin.copy(),
               outlier=None, round_flags=np.zeros((0, n), np.uint8), min_margin=math.inf, max_trials=0, empty_rounds=0)
    if n < 3:                                                    # if(nInitialCorrespondences<3) return 0;
        return out
    ev = make([np.float32(c) for c in cam], edges)
    order_all = list(range(n)) if sum_order is None else [int(i) for i in sum_order]
    assert sorted(order_all) == list(range(n))
    stereo = ~(edges["ur"] < 0)
    th = np.where(stereo, TH_STEREO, TH_MONO).astype(np.float32)
    flags = np.zeros(n, np.uint8)
    robust, T, rounds = True, None, []
    st = dict(lm_iterations=0, lm_trials=0, max_trials=0)
    for rnd in range(4):
        T = se3_from_pose(Tin)                                   # vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw))
        order = [i for i in order_all if not flags[i]]           # initializeOptimization(0)
        T_err = T
        if order:
            T, T_err = _levenberg(ev, T, order, robust, st)
        else:
            out["empty_rounds"] += 1                             # optimize() returns -1: nothing moves
        # an outlier gets computeError() at the estimate; an inlier keeps the error of the last computeActiveErrors() (D14)
        chi_now = ev.chi2_all(T)
        chi_err = chi_now if T_err is T else ev.chi2_all(T_err)
        with np.errstate(all="ignore"):
            chi = np.where(flags != 0, chi_now, chi_err).astype(np.float32)      # const float chi2 = e->chi2();
            margin = np.abs(chi.astype(np.float64) / th.astype(np.float64) - 1.0)
        if np.isfinite(margin).any():
            out["min_margin"] = min(out["min_margin"], float(np.nanmin(margin)))
        flags = (chi > th).astype(np.uint8)                      # NaN compares false: an inlier
        rounds.append(flags.copy())
        if rnd == 2:
            robust = False                                       # e->setRobustKernel(0)
        if n < 10:                                               # if(optimizer.edges().size()<10) break;
            break
    M = T.matrix()
    out.update(st)
    out.update(rounds=len(rounds), round_flags=np.array(rounds, np.uint8), outlier=flags, n_good=int(n - int(flags.sum())), Tcw_d=M,
               Tcw=M.astype(np.float32), status=STATUS_OK if np.isfinite(M).all() else STATUS_NONFINITE)
    return out


def pose_optimization_literal(Tcw, cam, edges, sum_order=None):
    return _pose_optimization(_Literal, Tcw, cam, edges, sum_order)


def pose_optimization_fast(Tcw, cam, edges, sum_order=None):
    return _pose_optimization(_Fast, Tcw, cam, edges, sum_order)


def gather_edges(kps, uR, kp_lm, lm_pos, size_ref=31.0, sigma_ref=1.0, cap=None):
    """the loop at Optimizer.cc:94-188 on arrays (hs_pose_edges_device): one edge per keypoint with 0 <= kp_lm < L, in ascending keypoint index.
    Returns (edges[:cap], full count)."""
    kp_lm = np.asarray(kp_lm, np.int32)
    L = len(lm_pos)
    idx = np.nonzero((kp_lm >= 0) & (kp_lm < L))[0]
    e = np.zeros(len(idx), EDGE_DTYPE)
    e["Xw"] = np.asarray(lm_pos, np.float32).reshape(-1, 3)[kp_lm[idx]]
    e["u"], e["v"], e["ur"] = kps["x"][idx], kps["y"][idx], np.asarray(uR, np.float32)[idx]
    e["inv_sigma2"] = inv_sigma2(kps["size"][idx], size_ref, sigma_ref)
    e["kp"] = idx
    return (e if cap is None else e[:cap]), len(idx)
