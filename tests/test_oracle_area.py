"""The grid-area matchers of the CPU oracle against the independent numpy restatement (tests/pyref.py), bit for bit, on generated edge cases
(tests/scenes.py area_edge_cases / area_size_cases) and on hand-built cases with known answers.  Covered: Frame::PosInGrid, the
GetFeaturesInArea cell walk (through every caller), SearchByProjection(pKF, Scw, ...) and SearchBySim3."""
import numpy as np
import pytest

import oracle
import pyref
import scenes

f32 = np.float32


def views(fa):
    F, keep = oracle.make_frame_view(oracle.FrameView, **fa)
    return F, keep


def check_case(case, sim3=True):
    fa = case["fa"]
    F, keep = views(fa)
    g = pyref.AreaGrid(fa["kps"], fa["bounds"])
    assert np.array_equal(oracle.frame_grid(F), g.cells), case["kind"]
    oi, ot, on = oracle.search_by_projection_sim3(F, case["Scw"], case["lms"], case["th"], case["th_low"], case["kp_matched"])
    pi, pt, pn = pyref.search_by_projection_sim3(fa, case["Scw"], case["lms"], case["th"], case["th_low"], case["kp_matched"], grid=g)
    assert np.array_equal(oi, pi) and np.array_equal(ot, pt) and on == pn, case["kind"]
    if not sim3:
        return on, 0
    s = case["sim3"]
    F2, keep2 = views(s["fb"])
    om, on2 = oracle.search_by_sim3(F, s["lms1"], F2, s["lms2"], s["s12"], s["R12"], s["t12"], s["th"], s["th_high"])
    pm, pn2 = pyref.search_by_sim3(fa, s["lms1"], s["fb"], s["lms2"], s["s12"], s["R12"], s["t12"], s["th"], s["th_high"],
                                   grids=(g, pyref.AreaGrid(s["fb"]["kps"], s["fb"]["bounds"])))
    assert np.array_equal(om, pm) and on2 == pn2, (case["kind"], "sim3")
    return on, on2


@pytest.mark.parametrize("block", range(6))
def test_generated_edge_cases_oracle_vs_pyref(block):
    """8 families x 60 seeds = 480 cases"""
    total = [0, 0]
    for seed in range(10 * block, 10 * block + 10):
        for case in scenes.area_edge_cases(seed):
            a, b = check_case(case)
            total[0] += a; total[1] += b
    assert total[0] > 200 and total[1] > 200, total                 # the cases are not all empty


def test_size_extremes_oracle_vs_pyref():
    for case in scenes.area_size_cases(5):
        check_case(case, sim3=len(case["fa"]["kps"]) <= 2000)


def frame(kps_xy, bounds=(0.0, 640.0, 0.0, 480.0), sizes=31.0, desc=None):
    from oracle import KP_DTYPE
    k = np.zeros(len(kps_xy), KP_DTYPE)
    if len(kps_xy):
        k["x"], k["y"] = np.asarray(kps_xy, f32).T
    k["size"] = sizes
    d = np.zeros((len(k), 32), np.uint8) if desc is None else desc
    return dict(Rcw=np.eye(3, dtype=f32), tcw=np.zeros(3, f32), fx=512.0, fy=512.0, cx=320.0, cy=240.0, mbf=51.2, sensor=1, bounds=bounds,
                kps=k, desc=d, uR=np.full(len(k), -1, f32), kp_lm_obs=np.full(len(k), -1, np.int32), size_ref=31.0)


def landmark(pos, size=0.1, assoc=-1, desc=None):
    lm = np.zeros(1, oracle.LM_DTYPE)
    lm["pos"] = pos
    p = np.asarray(pos, np.float64)
    d = np.linalg.norm(p)
    lm["size"], lm["assoc_kp"], lm["min_dist"], lm["max_dist"] = size, assoc, d * 0.5, d * 2
    lm["normal"] = p / d
    if desc is not None:
        lm["desc"] = desc
    return lm


def test_known_grid_cells():
    """PosInGrid rounds half away from zero; the last column rounds to 64 (outside); NaN, inf and 1e10 are outside (x86 conversion)"""
    cw = 10.0
    fa = frame([(4.99, 0), (5.0, 0), (635.0, 0), (634.99, 0), (640.0, 0), (np.nan, 10), (10, np.inf), (1e10, 5), (-1e10, 5), (-5.0, 0), (-4.99, 0)])
    F, keep = views(fa)
    want = [(0, 0), (1, 0), (-1, -1), (63, 0), (-1, -1), (-1, -1), (-1, -1), (-1, -1), (-1, -1), (-1, -1), (0, 0)]
    assert oracle.frame_grid(F).tolist() == [list(w) for w in want]
    assert pyref.frame_grid(fa["kps"], fa["bounds"]).tolist() == [list(w) for w in want]
    assert cw == 640.0 / 64


@pytest.mark.parametrize("size,want", [(4.0 * 31, 1), (1.0 * 31, -1), (3e10 * 31, -1), (np.inf, -1), (-31.0, -1), (np.nan, -1), (0.0, -1)])
def test_known_radius_answers(size, want):
    """A landmark projecting to (320, 240) with two keypoints: #0 (distance 0) exactly r = 4 to the right (strict: not a candidate) and #1
    (distance 1) 3.5 to the left.  Radius = th * size(assoc kp #2) / 31.  The radius 3e10 and +inf reach the int conversion's range: x86 gives
    INT_MIN, the cell range is empty and nothing matches."""
    d = np.zeros((3, 32), np.uint8); d[1, 0] = 1; d[2] = 0xFF
    fa = frame([(324.0, 240.0), (316.5, 240.0), (100.0, 100.0)], desc=d)
    fa["kps"]["size"][2] = size
    F, keep = views(fa)
    lms = landmark([0.0, 0.0, 2.0], assoc=2)
    for impl in (lambda: oracle.search_by_projection_sim3(F, np.eye(4, dtype=f32), lms, 1, 50.0, np.zeros(3, np.uint8)),
                 lambda: pyref.search_by_projection_sim3(fa, np.eye(4, dtype=f32), lms, 1, 50.0, np.zeros(3, np.uint8))):
        mi, taken, n = impl()
        assert mi.tolist() == [want], (size, mi)


def test_known_image_bounds_and_tie_order():
    """u == max_x exactly: KeyFrame::IsInImage (strict) rejects the landmark in SearchByProjection(pKF, Scw), Camera::Project (inclusive)
    keeps it in SearchBySim3.  Equal distances in cells (62, 24) and (63, 23): the column walk finds the lower column first."""
    # landmark at X/Z = 0.625 -> u = 512 * 0.625 + 320 = 640 = max_x; v = 240
    fa = frame([(632.0, 240.0), (634.0, 240.0)])
    F, keep = views(fa)
    lm = landmark([0.625, 0.0, 1.0], size=10.0)
    mi, _, n = oracle.search_by_projection_sim3(F, np.eye(4, dtype=f32), lm, 1, 50.0, np.zeros(2, np.uint8))
    assert mi.tolist() == [-1] and n == 0
    lms = np.concatenate([lm, lm]); lms["assoc_kp"] = -1
    om, on = oracle.search_by_sim3(F, lms, F, lms, 1.0, np.eye(3, dtype=f32), np.zeros(3, f32), 1.0, 100.0)
    pm, pn = pyref.search_by_sim3(fa, lms, fa, lms, 1.0, np.eye(3, dtype=f32), np.zeros(3, f32), 1.0, 100.0)
    assert om.tolist() == pm.tolist() and on == pn
    assert om.tolist() == [0, -1] and on == 1                 # both directions pick keypoint 0 (first of the tie), only landmark 0 agrees
    # ties across cells: #0 in cell (63, 23), #1 in cell (62, 24): the column-major walk visits (62, 24) first
    fa = frame([(630.0, 230.0), (620.0, 240.0)])
    F, keep = views(fa)
    lm = landmark([(625.0 - 320) / 512, (235.0 - 240) / 512, 1.0], size=20.0)
    for impl in (lambda: oracle.search_by_projection_sim3(F, np.eye(4, dtype=f32), lm, 1, 50.0, np.zeros(2, np.uint8)),
                 lambda: pyref.search_by_projection_sim3(fa, np.eye(4, dtype=f32), lm, 1, 50.0, np.zeros(2, np.uint8))):
        mi, taken, n = impl()
        assert mi.tolist() == [1] and taken.tolist() == [0, 1]


def test_known_sequential_assignment_and_threshold():
    """landmarks in order take keypoints: the second copy of a landmark gets the next best keypoint, a pre-matched keypoint is never taken,
    and a best distance equal to th_low matches (<=)"""
    d = np.zeros((3, 32), np.uint8)
    d[1, :6] = 0xFF; d[1, 6] = 0x03                                            # distance 50 to the zero descriptor
    d[2, :7] = 0xFF                                                            # distance 56
    fa = frame([(320.0, 240.0), (321.0, 240.0), (319.0, 241.0)], desc=d)
    F, keep = views(fa)
    lm = landmark([0.0, 0.0, 2.0], size=0.2)
    lms = np.concatenate([lm, lm, lm])
    for pre, want in (([0, 0, 0], [0, 1, -1]), ([1, 0, 0], [1, -1, -1])):
        pre = np.array(pre, np.uint8)
        for impl in (lambda: oracle.search_by_projection_sim3(F, np.eye(4, dtype=f32), lms, 3, 50.0, pre),
                     lambda: pyref.search_by_projection_sim3(fa, np.eye(4, dtype=f32), lms, 3, 50.0, pre)):
            mi, taken, n = impl()
            assert mi.tolist() == want and n == sum(w >= 0 for w in want)


def test_cvt_i32_models_x86():
    assert pyref.cvt_i32([np.nan, np.inf, -np.inf, 2147483648.0, -2147483648.0, 2147483520.0, -0.0, 3e10]).tolist() == \
        [pyref.INT_MIN, pyref.INT_MIN, pyref.INT_MIN, pyref.INT_MIN, pyref.INT_MIN, 2147483520, 0, pyref.INT_MIN]
