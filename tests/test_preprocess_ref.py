"""The two CPU references of ImageProcessing::PreProcessImg — the oracle (oracle/hs_oracle.cpp: preprocessImg, walks pixels) and the numpy restatement
(tests/pyref.py: preprocess, whole-frame arithmetic) — byte for byte on every case of tests/preprocess_cases.py, the table the GPU edge test runs too;
and hand-computed known answers for the branches tests/test_oracle_preprocess.py does not pin."""
import numpy as np
import pytest

import oracle
import preprocess_cases as P
import pyref


def test_the_table_holds_what_it_promises():
    """no empty output, every group present, every mode at every channel count, both near-half scales, every ow % 4 at a tight pitch"""
    assert {c["group"] for c in P.CASES.values()} == set(P.GROUPS)
    assert len(P.by_group("random")) == 200
    for c in P.CASES.values():
        assert c["ow"] >= 1 and c["oh"] >= 1, c["name"]
    assert {(c["cn"], c["mode"]) for c in P.CASES.values()} == {(cn, m) for cn in (1, 3, 4) for m in (0, 1, 2)}
    for s in (P.NEXT_BELOW_HALF, P.NEXT_ABOVE_HALF):
        assert s != 0.5 and any(c["scale"] == s and c["mode"] == 2 for c in P.CASES.values())
    for mode in (0, 1, 2):
        assert {c["ow"] % 4 for c in P.by_group("destination") if c["mode"] == mode and c["dst_pitch"] == c["ow"]} == {0, 1, 2, 3}
        assert {(c["cn"]) for c in P.by_group("quads") if c["mode"] == mode and c["ow"] > 256} == {1, 3, 4}
    area = {(c["w"], c["h"]) for c in P.by_group("area")}
    assert {(w, h) for w in P.AREA_SIZES for h in P.AREA_SIZES} <= area


@pytest.mark.parametrize("group", P.GROUPS)
def test_oracle_and_restatement_agree_on_every_case(group):
    cases = P.by_group(group)
    assert cases
    for c in cases:
        assert oracle.preprocess_size(c["w"], c["h"], c["scale"]) == (c["ow"], c["oh"]), c["name"]
        for rgb in c["orders"]:
            for i in range(c["batch"]):
                f = P.frame_of(c, i)
                a, b = oracle.preprocess(f, rgb, c["scale"]), pyref.preprocess(f, rgb, c["scale"])
                assert a.shape == b.shape == (c["oh"], c["ow"]), (c["name"], a.shape, b.shape)
                if not np.array_equal(a, b):
                    y, x = np.argwhere(a != b)[0]
                    raise AssertionError("%s rgb=%d image %d: first difference at row %d column %d: oracle %d, restatement %d" % (c["name"], rgb, i, y, x, a[y, x], b[y, x]))


def both(src, rgb, scale):
    a, b = oracle.preprocess(src, rgb, scale), pyref.preprocess(src, rgb, scale)
    assert np.array_equal(a, b)
    return a.tolist()


def test_known_answers_area_partial_blocks():
    # 3 x 3 at 0.5 -> cvRound(1.5) = 2 each way.  Block (0,0) is full: (10 + 20 + 40 + 51 + 2) >> 2 = 123 >> 2 = 30.  Block (0,1) has the two samples of
    # column 2: 2 and 3, float mean 2.5 -> 2 (half to even; (sum + 1) >> 1 would give 3).  Block (1,0) has the two samples of row 2: 6 and 9 -> 7.5 -> 8.
    # Block (1,1) has ONE sample, the corner: the mean of one value is the value.
    g = np.array([[10, 20, 2], [40, 51, 3], [6, 9, 201]], np.uint8)
    assert both(g, True, 0.5) == [[30, 2], [8, 201]]
    # the same corner in colour: the mean runs per channel, grey afterwards: (201 * 4899 + 7 * 9617 + 90 * 1868 + 8192) >> 14 = 1228330 >> 14 = 74
    c = np.zeros((3, 3, 3), np.uint8); c[2, 2] = (201, 7, 90)
    assert both(c, True, 0.5)[1][1] == (201 * 4899 + 7 * 9617 + 90 * 1868 + 8192) >> 14 == 74
    assert both(c, False, 0.5)[1][1] == (90 * 4899 + 7 * 9617 + 201 * 1868 + 8192) >> 14 == 54      # 891889 >> 14


def test_known_answers_area_dropped_column_and_row():
    # 5 wide at 0.5 -> cvRound(2.5) = 2 (half to even): columns 0..3 make the two blocks, column 4 belongs to no block and must not leak into block 1
    g = np.zeros((2, 5), np.uint8); g[:, 4] = 255
    assert both(g, True, 0.5) == [[0, 0]]
    g[:, 3] = 4                                                      # block 1 = (0 + 4 + 0 + 4 + 2) >> 2 = 2, still without column 4
    assert both(g, True, 0.5) == [[0, 2]]
    # and rows: 2 x 5 -> 1 x 2, row 4 dropped
    assert both(g.T.copy(), True, 0.5) == [[0], [2]]
    assert oracle.preprocess_size(9, 13, 0.5) == (4, 6)


def test_known_answers_upscale_by_3_borders():
    # 2 x 2 at 3.0 -> 6 x 6; 1 / scale = 1 / 3.  Per axis: d = 0 -> f = 0.5 / 3 - 0.5 = -1/3: floor -1, weight 2/3 — columns clamp to tap 0 with weight 0
    # (sx < 0), rows keep the weights and clip both rows to row 0; d = 1 -> f = 0: tap 0; d = 2 -> tap 0, weights (1365, 683) of 2048; d = 3 -> (683, 1365);
    # d = 4 -> f = 1: tap 1 is the last one (sx >= sw - 1: weight 0, the right tap is not read); d = 5 -> f = 4/3: the same.
    g = np.array([[0, 255], [255, 0]], np.uint8)
    out = both(g, True, 3.0)
    # the four corners have both clamps active and reproduce the source corners: row weights 683 + 1365 on the SAME row:
    # ((683 * (255 * 2048 >> 4)) >> 16) + ((1365 * (255 * 2048 >> 4)) >> 16) + 2 >> 2 = (340 + 679 + 2) >> 2 = 255
    assert ((683 * (255 * 2048 >> 4)) >> 16, (1365 * (255 * 2048 >> 4)) >> 16) == (340, 679)
    assert (out[0][0], out[0][5], out[5][0], out[5][5]) == (0, 255, 255, 0)
    assert out[0] == out[1] and out[4] == out[5] and [r[0] for r in out] == [r[1] for r in out] and [r[4] for r in out] == [r[5] for r in out]
    # an inner pixel (2, 2): h0 = 0 * 1365 + 255 * 683 = 174165, h1 = 255 * 1365 = 348075; >> 4: 10885, 21754;
    # (1365 * 10885) >> 16 = 226, (683 * 21754) >> 16 = 226; (226 + 226 + 2) >> 2 = 113
    assert ((1365 * (174165 >> 4)) >> 16, (683 * (348075 >> 4)) >> 16) == (226, 226)
    assert out[2][2] == 113 and out[3][3] == 113
    # the border row 0 between the clamps, (0, 2): both rows are row 0 = (0, 255): h = 255 * 683 = 174165 -> 10885; (683 * 10885) >> 16 = 113,
    # (1365 * 10885) >> 16 = 226; (113 + 226 + 2) >> 2 = 85 (255 / 3)
    assert out[0][2] == 85 and out[0][3] == (((683 * (255 * 1365 >> 4)) >> 16) + ((1365 * (255 * 1365 >> 4)) >> 16) + 2) >> 2 == 170


def test_known_answers_next_to_one_half():
    """The floats next to 0.5 take the bilinear path.  On a full 2x2 block the two paths agree while the weights are (1024, 1024): h = 1024 (a + b),
    (1024 * (h >> 4)) >> 16 = a + b exactly, so the result is (a + b + c + d + 2) >> 2 again.  They part where the drift of 1 / scale away from 2 has
    moved fx one float step off 0.5 and the weights are (1023, 1025); with the heavier tap on a 0 and the lighter one on 255 in both rows:
    h = 1023 * 255 = 260865, h >> 4 = 16304, (1024 * 16304) >> 16 = 254, (254 + 254 + 2) >> 2 = 127, where the rounded mean is (510 + 2) >> 2 = 128."""
    assert ((1024 * ((1023 * 255) >> 4)) >> 16, (254 + 254 + 2) >> 2, (255 + 255 + 2) >> 2) == (254, 127, 128)
    # below 0.5: 1 / scale = 2 + 1.19e-7.  dx = 4000: fx = 8000.5 + 4000.5 * 1.19e-7 = 8000.50048 -> the float 8000.5 + 2^-11: weights (1023, 1025), the
    # right tap is the heavier one
    g = np.full((2, 8008), 77, np.uint8)
    g[:, 8000], g[:, 8001] = 255, 0
    assert oracle.preprocess_size(8008, 2, P.NEXT_BELOW_HALF) == (4004, 1)
    assert both(g, True, P.NEXT_BELOW_HALF)[0][4000] == 127
    assert both(g[:, :8008], True, 0.5)[0][4000] == 128
    # above 0.5: 1 / scale = 2 - 2.38e-7.  dx = 2500: fx = 5000.5 - 2500.5 * 2.38e-7 = 5000.49940 -> the float 5000.5 - 2^-11: weights (1025, 1023), the
    # left tap is the heavier one
    g = np.full((2, 5008), 77, np.uint8)
    g[:, 5000], g[:, 5001] = 0, 255
    assert both(g, True, P.NEXT_ABOVE_HALF)[0][2500] == 127
    assert both(g, True, 0.5)[0][2500] == 128
    # and at the first block both give the rounded mean: nothing but the mode selection tells these scales from 0.5 on a small frame — except the
    # two-sample partial block, where the area path takes the float mean half to even and the bilinear path (a + b + 1) >> 1:
    g3 = np.array([[9, 9, 2], [9, 9, 3]], np.uint8)
    assert both(g3, True, 0.5) == [[9, 2]]
    assert both(g3, True, P.NEXT_ABOVE_HALF) == [[9, 3]]              # cvRound(3 * 0.50000006) = 2 as well
    assert oracle.preprocess_size(3, 2, P.NEXT_BELOW_HALF) == (1, 1)  # cvRound(1.4999999) = 1: the size itself differs from 0.5's


def test_known_answers_same_size_is_a_copy():
    rng = np.random.default_rng(11)
    f = rng.integers(0, 256, (35, 67), dtype=np.uint8)
    assert oracle.preprocess_size(67, 35, P.SAME_SIZE_SCALE) == (67, 35)
    assert both(f, True, P.SAME_SIZE_SCALE) == f.tolist()             # a bilinear pass at 1 / 0.999 would blend neighbours
