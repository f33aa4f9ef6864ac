"""Run by test_gpu_fast_scan_rows.py, one group of cases per process (the HS_FAST_* knobs are read when a handle is created): scan A of
k_fast_rows carries tile rows and vertical differences from one 8-row block of a wide item to the next.  Every case is compared with the
oracle bit for bit: the candidate sets per level and the final features (stage_parity), or the final features (assert_same_features)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle
import hyslam_amd as HS
from hyslam_amd.synth import synth_image
from test_gpu_parity import stage_parity, settings, assert_same_features


def textured(seed, w, h):
    """structure plus noise: corners of the synthetic scene and a noise floor that passes the quick reject here and there"""
    rng = np.random.default_rng(seed)
    return np.clip(synth_image(seed, w, h).astype(np.int32) + rng.integers(-14, 15, (h, w)), 0, 255).astype(np.uint8)


def item_heights(p, w, h, level):
    """interior rows of the items of one level, from the oracle's grid: hcell for every cell row but the last, which takes what is left"""
    lw, lh = oracle.pyramid_size(p, w, h, level)
    _, nrows, _, hcell = oracle.cell_grid(p, lw, lh)
    if nrows == 0:
        return []
    return [hcell] * (nrows - 1) + [(lh - 38) - hcell * (nrows - 1)]


def heights():
    """the last block of an item holds 8, 1, ... 7 valid rows: the cell height of every level moves through all residues mod 8"""
    seen = set()
    for h in range(150, 182):
        stage_parity(textured(h, 330, h), 600)
        seen |= {ih % 8 for ih in item_heights(oracle.default_params(600), 330, h, 0)}
    assert {0, 1, 7} <= seen, seen


def cells():
    """1 to 16 blocks per item: cells of 13, 25 and ~42 rows, and the tallest the library accepts (two cell rows of 125 and 119 pixel rows at level 0
    of the taller frame, ~100 and ~80 above it: the TR = 134 / 102 instances); upper levels and last cell rows supply the short items"""
    blocks = set()
    for n_cells, h, nlevels in ((12, 157, 8), (24, 157, 8), (40, 157, 8), (84, 282, 2)):     # (a third level of the last would hold a cell of 158 rows)
        img = textured(77 + n_cells, 330, h)
        p = oracle.default_params(800, 1.2, nlevels)
        p.cell_px = n_cells
        for level in range(p.nlevels):
            blocks |= {(ih + 7) // 8 for ih in item_heights(p, 330, h, level) if ih > 0}
        ok, od = oracle.extract(p, img)
        s = settings(800, 1.2, nlevels)
        s.N_CELLS = n_cells
        gk, gd = HS.ORBExtractor(s)(img)
        assert_same_features(gk, gd, ok, od)
    assert {1, 2, 4, 12, 13, 15, 16} <= blocks, blocks


def noise():
    """a saturated frame; with HS_FAST_TEST_SMALL_LISTS=1 the list overflows inside the scan: the corner pass runs between two blocks and corners spill"""
    img = np.random.default_rng(9).integers(0, 256, (240, 320), dtype=np.uint8)
    stage_parity(img, 1500)


def batch():
    """several items per persistent wave (three frames in one call; HS_FAST_NO_FOLD=1 puts the waves on the work queues): nothing carried from item to
    item.  With N_CELLS = 10 the last cell row of level 3 is a single pixel row."""
    frames = [textured(500 + i, 336, 200) for i in range(2)] + [np.random.default_rng(5).integers(0, 256, (200, 336), dtype=np.uint8)]
    for n_cells in (30, 10):
        p = oracle.default_params(700)
        p.cell_px = n_cells
        if n_cells == 10:
            assert item_heights(p, 336, 200, 3)[-1] == 1
        s = settings(700)
        s.N_CELLS = n_cells
        ex = HS.ORBExtractor(s)
        kl, dl = ex.extract_batch(frames)
        for f, gk, gd in zip(frames, kl, dl):
            ok, od = oracle.extract(p, f)
            assert_same_features(gk, gd, ok, od)


def thresholds():
    """other values of the per-byte bias of the reduced-precision compares"""
    img = textured(502, 336, 200)
    for t in (0, 3, 20, 100):
        p = oracle.default_params(700)
        p.fast_threshold = t
        ok, od = oracle.extract(p, img, cap=8000)
        gk, gd = HS.ORBExtractor(settings(700), fast_threshold=t)(img)
        assert_same_features(gk, gd, ok, od)


def narrow():
    """one frame per call without HS_FAST_COLS: the narrow items, whose scan is what it was"""
    assert "HS_FAST_COLS" not in os.environ
    stage_parity(textured(3, 640, 480), 1000)


if __name__ == "__main__":
    {"heights": heights, "cells": cells, "noise": noise, "batch": batch, "thresholds": thresholds, "narrow": narrow}[sys.argv[1]]()
    print("FAST_SCAN_ROWS_OK", sys.argv[1], {k: v for k, v in os.environ.items() if k.startswith("HS_")})
