"""Independent numpy restatement of the whole extractor (test infrastructure): how the primitives of tests/pyref.py are put together.

Written from the reference's src/features/ORBExtractor.cpp (constructor :76-119, ComputePyramid :564-589, ComputeKeyPointsOctTree :405-494,
operator() :496-562) and src/features/low_level/ORBFinder.cpp (setThreshold :58-60, detect :66-68, compute :70-78).  It imports nothing from
tests/oracle.py and never loads the oracle library: a misreading of the composition in oracle/hs_oracle.cpp (and in the kernels, which were
written by the same hand) shows up as a disagreement with this file.  The primitives (resize, FAST, blur, angle, descriptor, octtree) come
from pyref.  The 512-point sampling pattern is parsed from include/hyslam_orb_pattern.h: it is SHARED DATA, not independently pinned here
(tests/test_skimage_crosscheck.py pins it against scikit-image).

Float expressions are evaluated one float32 operation at a time, as the reference's x86-64 build does; `scaleFactor` is a double member
(ORBExtractor.h:116) that holds the float setting.  Slow (about 1 s for 640 x 480 at 1000 features); small frames only.
"""
import math
import os
import re

import numpy as np

import pyref

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])
PATCH_SIZE = 31                 # ORBExtractor.cpp:73
EDGE_THRESHOLD = 19             # ORBExtractor.cpp:74
_f = np.float32
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_pattern = None


def pattern():
    """the 1024 ints of bit_pattern_31_ (ORBFinder.cpp:151-409) as committed in include/hyslam_orb_pattern.h"""
    global _pattern
    if _pattern is None:
        text = open(os.path.join(_ROOT, "include", "hyslam_orb_pattern.h")).read()
        body = text[text.index("HS_ORB_PATTERN_INIT {") + len("HS_ORB_PATTERN_INIT {"):]
        body = body[:body.index("}")]
        v = np.array([int(t) for t in re.findall(r"-?\d+", body)], np.int64)
        assert len(v) == 1024, len(v)
        _pattern = v
    return _pattern


def tables(nfeatures, scale, nlevels):
    """The constructor's tables, ORBExtractor.cpp:86-117 -> (scale, inverse scale, sigma^2, inverse sigma^2, quotas)."""
    sf = np.float64(_f(scale))                                   # double scaleFactor = settings.fScaleFactor (a float), :81
    sc, s2 = np.zeros(nlevels, _f), np.zeros(nlevels, _f)
    sc[0] = s2[0] = 1                                            # :88-89
    for i in range(1, nlevels):
        sc[i] = _f(np.float64(sc[i - 1]) * sf)                   # :92 float * double, stored as float
        s2[i] = _f(sc[i] * sc[i])                                # :93
    isc = (_f(1) / sc).astype(_f)                                # :100
    is2 = (_f(1) / s2).astype(_f)                                # :101
    factor = _f(1.0 / sf)                                        # :107 float factor = 1.0f / scaleFactor (a double division)
    den = _f(_f(1) - _f(math.pow(float(factor), float(nlevels))))
    want = _f(_f(_f(nfeatures) * _f(_f(1) - factor)) / den)      # :108 int * float / float
    quotas = np.zeros(nlevels, np.int32)
    total = 0
    for level in range(nlevels - 1):                             # :111-116
        quotas[level] = int(np.rint(want))                       # cvRound: half to even
        total += int(quotas[level])
        want = _f(want * factor)
    quotas[nlevels - 1] = max(nfeatures - total, 0)              # :117
    return sc, isc, s2, is2, quotas


def level_sizes(w, h, scale, nlevels):
    """Size sz(cvRound((float)image.cols*scale), cvRound((float)image.rows*scale)) with scale = mvInvScaleFactor[level], :568-569 -> [(lw, lh)]"""
    isc = tables(1, scale, nlevels)[1]
    return [(int(np.rint(_f(_f(w) * isc[l]))), int(np.rint(_f(_f(h) * isc[l])))) for l in range(nlevels)]


def cell_grid(lw, lh, n_cells=30):
    """:413-428 -> (nCols, nRows, wCell, hCell).  N_CELLS is used as the cell edge in pixels (const float W = N_CELLS, :409).
    nCols == 0 (or nRows == 0) makes the reference divide by zero and convert the result to int, which is undefined; such a level runs no cell
    either way (the loops at :430 / :440 do not start), so the cell size is reported as 0."""
    min_b = EDGE_THRESHOLD - 3
    width, height = _f(lw - EDGE_THRESHOLD + 3 - min_b), _f(lh - EDGE_THRESHOLD + 3 - min_b)     # :422-423
    W = _f(n_cells)
    n_cols, n_rows = int(_f(width / W)), int(_f(height / W))     # :425-426, (int) truncates towards zero
    w_cell = int(math.ceil(_f(width / _f(n_cols)))) if n_cols > 0 else 0
    h_cell = int(math.ceil(_f(height / _f(n_rows)))) if n_rows > 0 else 0
    return n_cols, n_rows, w_cell, h_cell


def set_threshold(current, requested):
    """ORBFinder::setThreshold, ORBFinder.cpp:58-60: `threshold = static_cast<int>(std::round(threshold));` assigns the MEMBER to itself.  The
    argument is never read, so the finder keeps the 20 of its declaration (ORBFinder.h:92) through iniThFAST and minThFAST alike."""
    return int(round(current))


def level_candidates(level_img, n_cells=30, threshold=20, ini_threshold=20, min_threshold=4):
    """The cell loop, :411-470 -> (candidates float32 (n, 3): x, y, response relative to (minBorderX, minBorderY), in vToDistributeKeys order; stats)."""
    lh, lw = level_img.shape
    min_bx = min_by = EDGE_THRESHOLD - 3                         # :413-414
    max_bx, max_by = lw - EDGE_THRESHOLD + 3, lh - EDGE_THRESHOLD + 3
    n_cols, n_rows, w_cell, h_cell = cell_grid(lw, lh, n_cells)
    st = dict(cells_run=0, cells_retried=0, rows_skipped=0, cols_skipped=0, cells_skipped_row=0, cells_skipped_col=0, view_w=[], view_h=[],
              cell_of=[], grid=(n_cols, n_rows, w_cell, h_cell))
    out = []
    for i in range(max(n_rows, 0)):
        ini_y = min_by + i * h_cell                              # :432
        max_y = ini_y + h_cell + 6                               # :433
        if ini_y >= max_by - 3:                                  # :435
            st["rows_skipped"] += 1
            st["cells_skipped_row"] += max(n_cols, 0)
            continue
        max_y = min(max_y, max_by)                               # :437-438
        skipped_here = 0
        for j in range(max(n_cols, 0)):
            ini_x = min_bx + j * w_cell                          # :442
            max_x = ini_x + w_cell + 6                           # :443
            if ini_x >= max_bx - 6:                              # :444
                st["cells_skipped_col"] += 1
                skipped_here += 1
                continue
            max_x = min(max_x, max_bx)                           # :446-447
            view = level_img[ini_y:max_y, ini_x:max_x]           # rowRange(iniY, maxY).colRange(iniX, maxX), :451
            st["cells_run"] += 1
            st["view_w"].append(max_x - ini_x)
            st["view_h"].append(max_y - ini_y)
            t = set_threshold(threshold, ini_threshold)          # :450
            keys = pyref.fast(view, t, True)                     # cv::FAST(image, keypoints, threshold, non_max_suppression), ORBFinder.cpp:67
            if len(keys) == 0:                                   # :453-457
                st["cells_retried"] += 1
                t2 = set_threshold(t, min_threshold)
                if t2 != t:                                      # the same view at the same threshold is empty again
                    keys = pyref.fast(view, t2, True)
            for x, y, s in keys:                                 # :461-466, cv::FAST's order: rows top down, columns left to right
                out.append((_f(_f(x) + _f(j * w_cell)), _f(_f(y) + _f(i * h_cell)), _f(s)))
                st["cell_of"].append((i, j))
        st["cols_skipped"] = max(st["cols_skipped"], skipped_here)
    return np.array(out, _f).reshape(-1, 3), st


def extract(img, nfeatures, scale, nlevels, n_cells=30, fast_threshold=20, blur_taps=None, debug=False, min_threshold=4):
    """ORBExtractor::operator(), :496-562 -> (keypoints KP_DTYPE [n], descriptors uint8 (n, 32)[, debug dict]).
    debug: pyramid / blurred (every level), candidates (float32 (n, 3) per level), selected (float32 (n, 3) per level: x, y, response in level
    pixels, border added, in DistributeOctTree's result order), n_selected, stats (per level, see level_candidates), quotas, scale."""
    img = np.ascontiguousarray(img, np.uint8)
    if img.size == 0:                                            # :499-500
        e = (np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8))
        return e + (dict(pyramid=[], blurred=[], candidates=[], selected=[], n_selected=[], stats=[]),) if debug else e
    taps = pyref.TAPS if blur_taps is None or not any(blur_taps) else np.asarray(blur_taps, np.int64)
    sc, isc, _, _, quotas = tables(nfeatures, scale, nlevels)
    h, w = img.shape
    sizes = level_sizes(w, h, scale, nlevels)
    # ---- ComputePyramid, :564-589.  The EDGE_THRESHOLD border that copyMakeBorder adds around every level is never read: FAST views stay inside
    # [16, size - 16) and the descriptors are computed on a clone of the level itself (:536), so levels are kept without it.
    pyr = []
    for level, (lw, lh) in enumerate(sizes):
        if lw < 1 or lh < 1:
            raise ValueError("pyramid level %d collapses to %d x %d" % (level, lw, lh))
        pyr.append(img if level == 0 else pyref.resize_linear(pyr[level - 1], lw, lh))      # :577 from level-1, INTER_LINEAR
    # ---- ComputeKeyPointsOctTree, :405-494
    cands, sel, stats = [], [], []
    for level, (lw, lh) in enumerate(sizes):
        min_b = EDGE_THRESHOLD - 3
        max_bx, max_by = lw - EDGE_THRESHOLD + 3, lh - EDGE_THRESHOLD + 3
        c, st = level_candidates(pyr[level], n_cells, fast_threshold, min_threshold=min_threshold)
        cands.append(c)
        stats.append(st)
        keep = pyref.distribute_octtree(c.tolist(), min_b, max_bx, min_b, max_by, int(quotas[level])) if len(c) else []     # :475-476
        k = c[keep].reshape(-1, 3).copy()
        k[:, 0] = (k[:, 0] + _f(min_b)).astype(_f)               # :484-485
        k[:, 1] = (k[:, 1] + _f(min_b)).astype(_f)
        sel.append(k)
    # ---- operator(), :513-555: levels in order, empty ones skipped
    pat = pattern()
    kps, desc, blurred = [], [], [None] * nlevels
    for level in range(nlevels):
        k = sel[level]
        if len(k) == 0:                                          # :532-533
            if debug:
                blurred[level] = pyref.gaussian_blur7(pyr[level], taps)
            continue
        work = pyref.gaussian_blur7(pyr[level], taps)            # :536-537 GaussianBlur(7x7, sigma 2, BORDER_REFLECT_101)
        blurred[level] = work
        rec = np.zeros(len(k), KP_DTYPE)
        d = np.zeros((len(k), 32), np.uint8)
        for i, (x, y, r) in enumerate(k):                        # ORBFinder::compute, ORBFinder.cpp:70-78: all angles, then all descriptors
            a = pyref.ic_angle(work, x, y)
            d[i] = pyref.orb_descriptor(work, x, y, a, pat)
            rec[i] = (x, y, 0, a, r, level)
        rec["size"] = _f(int(_f(_f(PATCH_SIZE) * sc[level])))    # const int scaledPatchSize = PATCH_SIZE*mvScaleFactor[level], :478, :487
        if level != 0:                                           # :546-552 keypoint->pt *= scale
            rec["x"] = (rec["x"] * sc[level]).astype(_f)
            rec["y"] = (rec["y"] * sc[level]).astype(_f)
        kps.append(rec)
        desc.append(d)
    K = np.concatenate(kps) if kps else np.zeros(0, KP_DTYPE)
    D = np.concatenate(desc) if desc else np.zeros((0, 32), np.uint8)
    if not debug:
        return K, D
    return K, D, dict(pyramid=pyr, blurred=blurred, candidates=cands, selected=sel, n_selected=[len(s) for s in sel], stats=stats,
                      quotas=quotas, scale=sc)


def extract_camera(frame, rgb, camera_scale, nfeatures, scale, nlevels, **kw):
    """ImageProcessing::PreProcessImg (src/main/ImageProcessing.cpp:118-138) in front of the extractor, as ProcessMonoImage calls them (:44, :55)
    -> (grey frame, keypoints, descriptors)"""
    grey = pyref.preprocess(np.asarray(frame, np.uint8), rgb, camera_scale)
    k, d = extract(grey, nfeatures, scale, nlevels, **kw)
    return grey, k, d


def stereo_frontend(img_left, img_right, nfeatures, scale, nlevels, fx, mbf, n_rows, th_high=100.0, th_low=50.0, size_ref=31.0, **kw):
    """ImageProcessing::ProcessStereoImage (src/main/ImageProcessing.cpp:69-116): both views through their own extractor, then
    Stereomatcher::computeStereoMatches -> (kL, dL, kR, dR, uRight, depth)"""
    kL, dL = extract(img_left, nfeatures, scale, nlevels, **kw)
    kR, dR = extract(img_right, nfeatures, scale, nlevels, **kw)
    u, z, _, _ = pyref.stereo_match(kL, dL, kR, dR, fx, mbf, n_rows, th_high, th_low, size_ref)
    return kL, dL, kR, dR, u, z
