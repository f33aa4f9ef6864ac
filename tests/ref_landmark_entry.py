"""Independent restatement of MapPointDBEntry::_updateEntry_ (reference: src/core/MapPointDB.cpp:223-310) in numpy scalar steps, written from the
reference's text and DESIGN.md D8 (OpenCV 3.4's arithmetic under the reference's cv::Mat expressions):
  _updateNormalAndDepth_ (:230-265)      normal = sum of (Pos - Ow_o) / cv::norm(Pos - Ow_o), then / n; depth range from the reference key frame
  _computeDistinctiveDescriptor_ (:128)  ref_landmark.distinctive_descriptor over the separate descriptor set
  _updateMeanDistance_ (:267-289)        float sum of the float norms, / (float)N
  _updateSize_ (:291-310)                KeyFrame::featureSizeMetric (KeyFrame.cc:234-255) + Camera::Unproject (Camera.cpp:155-159), the values > 0 summed,
                                         / (float)n — no early return, so 0.0f / 0.0f = NaN without a positive size
Every arithmetic step that D8 names is a method of Ops, so tests/test_landmark_entry_ref.py can swap one step for a mutant.
update_entries_fast computes the same answers vectorised over observations (elementwise numpy float32 / float64 rounds like the scalar steps;
the order-dependent sums walk observation positions one at a time) for the large GPU batches; the CPU tests pin it to update_entry."""
import numpy as np

from ref_landmark import distinctive_descriptor, distinctive_descriptors_fast

f32, f64 = np.float32, np.float64
HS_LM_SET_NORMAL_DEPTH, HS_LM_SET_DESC, HS_LM_SET_MEAN, HS_LM_SET_SIZE = 1, 2, 4, 8


class Ops:
    @staticmethod
    def norm(v):
        """cv::norm of a continuous 3x1 CV_32F: sum of (double)v_k * v_k left to right (from 0), std::sqrt in double; a double"""
        s = f64(0.0)
        for x in v:
            x = f64(f32(x))
            s = s + x * x
        return np.sqrt(s)

    @staticmethod
    def alpha(s):
        """normali / cv::norm(normali) is a MatExpr with alpha = 1.0/s (double); cv::scaleAdd rounds alpha to float for CV_32F"""
        return f32(f64(1.0) / s)

    @staticmethod
    def scale_add(d, a, acc):
        """scaleAdd_32f: dst = src1*alpha + src2, two float roundings"""
        return f32(d * a) + acc

    @staticmethod
    def divide(x, n):
        """normal / n: MatOp_AddEx::assign.  n >= 2: convertTo(alpha = 1.0/n, beta = 0) = fl(fl(x * (float)alpha) + 0.0f).  n == 1: |alpha| == 1
        into an empty Mat, so cv::add(a, Scalar(0)) = fl(x + 0.0f) — the same value, since x * 1.0f == x (D8)"""
        if n == 1:
            return x + f32(0.0)
        return f32(x * f32(f64(1.0) / f64(n))) + f32(0.0)

    @staticmethod
    def positive(s):
        return s > 0.0                                                    # `size_this > 0.0` (:298)

    @staticmethod
    def total(values):
        """mean_dist += this_dist / mean_size += size_this: float, strictly in observation order"""
        t = f32(0.0)
        for v in values:
            t = t + f32(v)
        return t

    size_returns_early = False                                            # _updateSize_ has no `if (observations.empty()) return;`


def sub3(a, b):
    return [f32(a[k]) - f32(b[k]) for k in range(3)]


def feature_size_metric(o, ops=Ops):
    """KeyFrame::featureSizeMetric(idx) for one observation record (LM_OBS_DTYPE fields)"""
    if not o["assoc"]:
        return f32(-1.0)
    z = f32(ops.norm(sub3(o["assoc_pos"], o["Ow"])))
    if z < 0.0:
        return f32(-1.0)
    u, v = f32(o["u"]), f32(o["v"])
    radius = f32(o["kp_size"]) / f32(2)
    fx, fy, cx, cy = f32(o["fx"]), f32(o["fy"]), f32(o["cx"]), f32(o["cy"])

    def unproject(uu, vv, zz):                                            # Camera::Unproject
        return [(uu - cx) * (zz / fx), (vv - cy) * (zz / fy), zz]

    left, right = unproject(u - radius, v, z), unproject(u + radius, v, z)
    return f32(ops.norm(sub3(right, left)))


def update_entry(pos, ref_Ow, obs, descs, max_factor=2.0, min_factor=0.5, ops=Ops):
    """one landmark.  obs: a sequence of LM_OBS_DTYPE records in the reference's std::map order; descs: (M, 32) uint8.
    Returns a dict: normal (3 float32) / min_dist / max_dist / mean_dist = None where the reference leaves them unchanged, size, best, median, flags."""
    with np.errstate(all="ignore"):
        r = dict(normal=None, min_dist=None, max_dist=None, mean_dist=None)
        N = len(obs)
        if N > 0:                                                         # _updateNormalAndDepth_
            normal = [f32(0.0)] * 3
            n = 0
            for o in obs:
                d = sub3(pos, o["Ow"])
                a = ops.alpha(ops.norm(d))
                normal = [ops.scale_add(d[k], a, normal[k]) for k in range(3)]
                n += 1
            dist = f32(ops.norm(sub3(pos, ref_Ow)))
            r["max_dist"], r["min_dist"] = f32(max_factor) * dist, f32(min_factor) * dist
            r["normal"] = [ops.divide(x, n) for x in normal]
        r["best"], r["median"] = distinctive_descriptor(descs)
        if N > 0:                                                         # _updateMeanDistance_
            r["mean_dist"] = ops.total([f32(ops.norm(sub3(pos, o["Ow"]))) for o in obs]) / f32(N)
        sizes = [feature_size_metric(o, ops) for o in obs]                # _updateSize_
        kept = [s for s in sizes if ops.positive(s)]
        r["size"] = None if (ops.size_returns_early and N == 0) else ops.total(kept) / f32(len(kept))
        r["flags"] = ((HS_LM_SET_NORMAL_DEPTH | HS_LM_SET_MEAN) if N > 0 else 0) | (HS_LM_SET_DESC if r["best"] >= 0 else 0) | \
            (HS_LM_SET_SIZE if r["size"] is not None else 0)
    return r


def update_entries(entries, obs_lists, desc_lists, max_factor=2.0, min_factor=0.5, ops=Ops):
    """a batch through update_entry -> dict of arrays like FeatureMatcher.UpdateLandmarkEntries (NaN where an output is not set)"""
    rs = [update_entry(e["pos"], e["ref_Ow"], o, d, max_factor, min_factor, ops) for e, o, d in zip(entries, obs_lists, desc_lists)]
    return _collect(rs)


def _collect(rs):
    L = len(rs)
    out = dict(normal=np.full((L, 3), np.nan, f32), min_dist=np.full(L, np.nan, f32), max_dist=np.full(L, np.nan, f32),
               mean_dist=np.full(L, np.nan, f32), size=np.full(L, np.nan, f32), best=np.zeros(L, np.int32), median=np.zeros(L, np.int32),
               flags=np.zeros(L, np.int32))
    for i, r in enumerate(rs):
        for k in ("min_dist", "max_dist", "mean_dist", "size"):
            if r[k] is not None:
                out[k][i] = r[k]
        if r["normal"] is not None:
            out["normal"][i] = r["normal"]
        out["best"][i], out["median"][i], out["flags"][i] = r["best"], r["median"], r["flags"]
    return out


def _norm_v(x, y, z):
    x, y, z = x.astype(f64), y.astype(f64), z.astype(f64)
    return np.sqrt(((f64(0.0) + x * x) + y * y) + z * z)


def update_entries_fast(entries, obs_offsets, obs, desc_lists, max_factor=2.0, min_factor=0.5):
    """update_entries on CSR observations, vectorised (same roundings; sums in observation order)"""
    with np.errstate(all="ignore"):
        ent = np.asarray(entries)
        L = len(ent)
        off = np.asarray(obs_offsets, np.int64)
        cnt = np.diff(off)
        owner = np.repeat(np.arange(L), cnt)
        pos = ent["pos"].astype(f32)[owner]
        Ow = obs["Ow"].astype(f32)
        d = pos - Ow
        s = _norm_v(d[:, 0], d[:, 1], d[:, 2])
        alpha = (f64(1.0) / s).astype(f32)
        term = d * alpha[:, None]
        dist_o = s.astype(f32)
        # featureSizeMetric
        P = obs["assoc_pos"].astype(f32) - Ow
        z = _norm_v(P[:, 0], P[:, 1], P[:, 2]).astype(f32)
        r = obs["kp_size"].astype(f32) / f32(2)
        u, v = obs["u"].astype(f32), obs["v"].astype(f32)
        zx, zy = z / obs["fx"].astype(f32), z / obs["fy"].astype(f32)
        xl, xr = (u - r - obs["cx"]) * zx, (u + r - obs["cx"]) * zx
        yl = yr = (v - obs["cy"].astype(f32)) * zy
        sz = _norm_v(xr - xl, yr - yl, z - z).astype(f32)
        sz = np.where((obs["assoc"] != 0) & ~(z < 0), sz, f32(-1.0))
        # order-dependent sums: position k of every landmark that has one, k = 0, 1, ...
        normal = np.zeros((L, 3), f32)
        mean = np.zeros(L, f32)
        ssum = np.zeros(L, f32)
        npos = np.zeros(L, np.int64)
        for k in range(int(cnt.max()) if L else 0):
            li = np.nonzero(cnt > k)[0]
            j = off[li] + k
            normal[li] = term[j] + normal[li]
            mean[li] = mean[li] + dist_o[j]
            ok = sz[j] > 0.0
            ssum[li[ok]] = ssum[li[ok]] + sz[j[ok]]
            npos[li[ok]] += 1
        has = cnt > 0
        an = np.where(has, (f64(1.0) / np.maximum(cnt, 1)).astype(f32), f32(1.0))
        normal = (normal * an[:, None]) + f32(0.0)
        dr = ent["pos"].astype(f32) - ent["ref_Ow"].astype(f32)
        dref = _norm_v(dr[:, 0], dr[:, 1], dr[:, 2]).astype(f32)
        out = dict(normal=np.where(has[:, None], normal, f32(np.nan)).astype(f32),
                   min_dist=np.where(has, f32(min_factor) * dref, f32(np.nan)).astype(f32),
                   max_dist=np.where(has, f32(max_factor) * dref, f32(np.nan)).astype(f32),
                   mean_dist=np.where(has, mean / cnt.astype(f32), f32(np.nan)).astype(f32),
                   size=(ssum / npos.astype(f32)).astype(f32))
        out["best"], out["median"] = distinctive_descriptors_fast(desc_lists)
        out["flags"] = (np.where(has, HS_LM_SET_NORMAL_DEPTH | HS_LM_SET_MEAN, 0) | np.where(out["best"] >= 0, HS_LM_SET_DESC, 0) |
                        HS_LM_SET_SIZE).astype(np.int32)
    return out


def same(a, b):
    """bit-exact, except that a NaN only has to meet a NaN (sign and payload are not specified)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))
