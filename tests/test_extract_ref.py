"""The C++ oracle's extractor against the independent numpy restatement of the whole composition (tests/ref_extract.py) on the directed scenes of
tests/extract_cases.py: every witness true, every stage bit for bit.  CPU only."""
import numpy as np
import pytest

import extract_cases as X
import oracle
import ref_extract as R
from hyslam_amd import _native as N


def oracle_params(nfeatures, scale, nlevels, n_cells=30, fast_threshold=20, blur_taps=None):
    p = oracle.default_params(nfeatures, scale, nlevels)
    p.cell_px, p.fast_threshold = n_cells, fast_threshold
    if blur_taps is not None:
        for i, t in enumerate(blur_taps):
            p.blur_taps[i] = int(t)
    return p


def test_keypoint_layout():
    assert R.KP_DTYPE == N.KP_DTYPE == oracle.KP_DTYPE
    assert np.array_equal(R.pattern(), oracle.pattern())          # shared data: the same table on both sides


@pytest.mark.parametrize("name", list(X.CASES))
def test_case_witness_and_oracle_parity(name):
    c = X.CASES[name]
    rk, rd, g = X.reference(name)
    for label, ok in c["witness"](rk, rd, g):
        assert ok, "%s: witness false: %s" % (name, label)
    ok_, od, dbg = oracle.extract(oracle_params(**X.settings_of(c)), c["img"], debug=True)
    L = c["nlevels"]
    for l in range(L):
        assert np.array_equal(dbg["pyramid"][l], g["pyramid"][l]), (name, "pyramid", l)
        assert dbg["candidates"][l].tobytes() == g["candidates"][l].tobytes(), (name, "candidates", l, len(dbg["candidates"][l]), len(g["candidates"][l]))
        assert int(dbg["n_selected"][l]) == g["n_selected"][l], (name, "selection count", l)
        assert np.array_equal(dbg["blurred"][l], g["blurred"][l]), (name, "blurred", l)
    assert len(ok_) == len(rk), (name, len(ok_), len(rk))
    assert ok_.tobytes() == rk.tobytes(), name
    assert np.array_equal(od, rd), name
    k2, d2 = R.extract(c["img"], **X.settings_of(c)) if name == "plain_161x123" else (rk, rd)          # the plain return of extract() is the debug one's
    assert k2.tobytes() == rk.tobytes() and np.array_equal(d2, rd)


@pytest.mark.parametrize("scale", X.QUOTA_SCALES)
def test_scale_tables_over_the_quota_grid(scale):
    ties = clamped = overshoot = 0
    for L in X.QUOTA_LEVELS:
        for nf in X.QUOTA_NFEATURES:
            ref = R.tables(nf, scale, L)
            got = oracle.scale_tables(oracle.default_params(nf, scale, L))
            for a, b in zip(ref, got):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (nf, scale, L)
            clamped += int(ref[4][-1] == 0)
            overshoot += int(ref[4][:-1].sum() > nf)
            f = np.float32
            factor = f(1.0 / np.float64(f(scale)))
            want = f(f(f(nf) * f(f(1) - factor)) / f(f(1) - f(float(factor) ** L)))
            for _ in range(L - 1):
                ties += int(want - np.floor(want) == f(0.5))
                want = f(want * factor)
    # witnesses of the grid itself: a last level clamped to 0 at every scale; cvRound on an exact .5 and an overshoot (max(..., 0) binding) where they exist
    assert clamped > 0, scale
    if scale in (1.1, 1.2, 1.25, 1.4, 1.7):
        assert ties > 0 and overshoot > 0, (scale, ties, overshoot)
    if scale == 2.0:
        assert ties > 0, scale


def test_level_sizes_and_cell_grid_over_the_size_grid():
    sizes = sorted(set(list(range(1, 70)) + list(range(70, 700, 7)) + [97, 83, 209, 225, 241, 273, 320, 240, 640, 480, 643, 481, 752, 1241, 1920, 1080]))
    for scale in X.QUOTA_SCALES:
        for L in (1, 3, 8, 12):
            p = oracle.default_params(100, scale, L)
            for e in sizes:
                ref = R.level_sizes(e, sizes[(sizes.index(e) * 7 + 3) % len(sizes)], scale, L)
                for l in range(L):
                    assert oracle.pyramid_size(p, e, sizes[(sizes.index(e) * 7 + 3) % len(sizes)], l) == ref[l], (scale, L, e, l)
    for cells in (8, 16, 24, 30, 37, 48):
        p = oracle.default_params(100)
        p.cell_px = cells
        for e in range(1, 800):
            o = 800 - e
            assert oracle.cell_grid(p, e, o) == R.cell_grid(e, o, cells), (cells, e, o)


def test_stereo_front_end():
    kw = X.STEREO
    p = oracle_params(kw["nfeatures"], kw["scale"], kw["nlevels"], kw["n_cells"])
    sp = oracle.stereo_params(fx=kw["fx"], mbf=kw["mbf"], n_rows=kw["n_rows"])
    L, Rt = X.stereo_pairs()[0]
    got = oracle.stereo_frontend(p, sp, L, Rt)
    ref = X.stereo_reference(0)
    assert len(ref[0]) > 200 and int((ref[5] > 0).sum()) > 30
    for a, b in zip(got, ref):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("scale", X.CAMERA_SCALES)
def test_camera_frame_front_end(scale):
    kw = X.CAMERA
    frame = X.colour_frame(71)
    grey, rk, rd = X.camera_reference(scale)
    og = oracle.preprocess(frame, False, scale)
    assert og.shape == (round(360 * scale), round(480 * scale)) and np.array_equal(og, grey)
    ok_, od = oracle.extract(oracle_params(kw["nfeatures"], kw["scale"], kw["nlevels"], kw["n_cells"]), og)
    assert len(rk) > 200 and ok_.tobytes() == rk.tobytes() and np.array_equal(od, rd)
