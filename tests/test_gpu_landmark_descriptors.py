"""GPU: hs_landmark_best_descriptors(_device) — MapPointDBEntry::_computeDistinctiveDescriptor_ (src/core/MapPointDB.cpp:128-175) for a batch —
bit-exact `best` and `median` against the restatement in tests/ref_landmark.py (pinned by tests/test_landmark_ref.py), through the C ABI, the Python
method FeatureMatcher.ComputeDistinctiveDescriptors and the C++ adaptor hyslam_amd/host/HipLandmarkDescriptors.h."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hipmem
from landmark_cases import KNOWN
from ref_landmark import distinctive_descriptors, distinctive_descriptors_fast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
EXE = os.path.join(BUILD, "test_landmark_adaptor")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(gpu):
    import hyslam_amd as HS
    return HS.FeatureMatcher(extractor=HS.ORBExtractor(device=0))


def clustered(rng, n, centres=3, max_flips=3):
    """n observations around a few centre descriptors with 0..max_flips flipped bits: duplicates and tied medians are common"""
    base = rng.integers(0, 256, (centres, 32), dtype=np.uint8)
    d = base[rng.integers(0, centres, n)].copy()
    for k in range(n):
        for f in rng.integers(0, 256, int(rng.integers(0, max_flips + 1))):
            d[k, f // 8] ^= np.uint8(1 << (f % 8))
    return d


def csr(landmarks):
    off = np.zeros(len(landmarks) + 1, np.int64)
    np.cumsum([len(d) for d in landmarks], out=off[1:])
    desc = np.concatenate([np.asarray(d, np.uint8).reshape(-1, 32) for d in landmarks]) if landmarks else np.zeros((0, 32), np.uint8)
    return off, np.ascontiguousarray(desc)


def ragged_batch(seed, L, big=(), n_max=40):
    rng = np.random.default_rng(seed)
    lms = []
    for i in range(L):
        n = int(rng.integers(2, n_max + 1)) if i % 50 else int(rng.integers(0, 2))          # N from 2..n_max, with some 0s and 1s
        lms.append(clustered(rng, n, centres=int(rng.integers(1, 4))) if i % 3 else rng.integers(0, 256, (n, 32), dtype=np.uint8))
    for pos, n in big:
        lms[pos] = clustered(rng, n, centres=4, max_flips=6)
    return lms


def test_known_answers(matcher):
    names = sorted(KNOWN)
    b, m = matcher.ComputeDistinctiveDescriptors([KNOWN[k][0] for k in names])
    assert b.tolist() == [KNOWN[k][1] for k in names] and m.tolist() == [KNOWN[k][2] for k in names], list(zip(names, b, m))


def test_known_answers_on_the_large_path(matcher):
    """the known cases through the workgroup path: each one repeated end to end until N > 64 (ties between the copies: the first copy wins)"""
    lms = [np.concatenate([KNOWN[k][0]] * (64 // len(KNOWN[k][0]) + 1)) for k in sorted(KNOWN)]
    assert min(len(d) for d in lms) > 64
    b, m = matcher.ComputeDistinctiveDescriptors(lms)
    rb, rm = distinctive_descriptors(lms)
    assert np.array_equal(b, rb) and np.array_equal(m, rm)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 1000, 5000])
def test_every_path_boundary(matcher, n):
    rng = np.random.default_rng(1000 + n)
    lms = [rng.integers(0, 256, (n, 32), dtype=np.uint8), clustered(rng, n), clustered(rng, n, centres=1, max_flips=1), np.tile(rng.integers(0, 256, (1, 32), dtype=np.uint8), (n, 1))]
    b, m = matcher.ComputeDistinctiveDescriptors(lms)
    rb, rm = distinctive_descriptors_fast(lms)
    assert np.array_equal(b, rb) and np.array_equal(m, rm), (n, b, rb, m, rm)


def test_median_256_row_on_both_paths(matcher):
    """a row whose median is 256 (one descriptor against many copies of its complement): bin 256 of the large path's histogram"""
    a = np.zeros(32, np.uint8)
    lms = [np.stack([a] + [~a] * n) for n in (2, 40, 64, 65, 300)]
    lms += [np.stack([~a] * n + [a]) for n in (40, 300)]
    b, m = matcher.ComputeDistinctiveDescriptors(lms)
    rb, rm = distinctive_descriptors(lms)
    assert np.array_equal(b, rb) and np.array_equal(m, rm)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_ragged_batches(matcher, seed):
    lms = ragged_batch(seed, 20000, big=[(17, 500), (9000, 700), (19999, 65)])
    b, m = matcher.ComputeDistinctiveDescriptors(lms)
    rb, rm = distinctive_descriptors_fast(lms)
    bad = np.nonzero((b != rb) | (m != rm))[0]
    assert len(bad) == 0, [(int(i), len(lms[i]), int(b[i]), int(rb[i]), int(m[i]), int(rm[i])) for i in bad[:10]]
    # the CSR form of the same batch gives the same answer
    off, desc = csr(lms)
    b2, m2 = matcher.ComputeDistinctiveDescriptors(offsets=off, desc=desc)
    assert np.array_equal(b2, b) and np.array_equal(m2, m)


def test_empty_batch_and_empty_landmarks(matcher):
    b, m = matcher.ComputeDistinctiveDescriptors([])
    assert len(b) == 0 and len(m) == 0
    b, m = matcher.ComputeDistinctiveDescriptors(offsets=np.zeros(1, np.int64), desc=np.zeros((0, 32), np.uint8))
    assert len(b) == 0
    b, m = matcher.ComputeDistinctiveDescriptors([np.zeros((0, 32), np.uint8)] * 3)
    assert b.tolist() == [-1] * 3 and m.tolist() == [-1] * 3


def test_csr_offsets_need_not_start_at_zero(matcher):
    """offsets index straight into desc: leading descriptors no landmark owns are skipped"""
    rng = np.random.default_rng(7)
    lms = ragged_batch(7, 200, big=[(5, 90)])
    off, desc = csr(lms)
    junk = rng.integers(0, 256, (13, 32), dtype=np.uint8)
    b, m = matcher.ComputeDistinctiveDescriptors(offsets=off + 13, desc=np.concatenate([junk, desc]))
    rb, rm = distinctive_descriptors_fast(lms)
    assert np.array_equal(b, rb) and np.array_equal(m, rm)


def test_bad_offsets_are_refused(matcher):
    from hyslam_amd import _native as N
    ex = matcher._ex
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    desc = np.zeros((10, 32), np.uint8)
    best, med = np.zeros(2, np.int32), np.zeros(2, np.int32)
    for off in ([0, 5, 3], [-1, 2, 4]):
        o = np.array(off, np.int64)
        assert ex._lib.hs_landmark_best_descriptors(ex._h, p(o), p(desc), 2, p(best), p(med)) == N.HS_ERR_INVALID
    assert ex._lib.hs_landmark_best_descriptors(ex._h, None, None, 0, None, None) == N.HS_OK
    assert ex._lib.hs_landmark_best_descriptors(ex._h, None, p(desc), 2, p(best), p(med)) == N.HS_ERR_INVALID


def test_host_entry_point_reuses_its_handle_across_sizes(matcher):
    """one handle, a large, a small and a larger batch: the scratch grows and is reused without stale results"""
    for seed, L in ((20, 5000), (21, 7), (22, 12000)):
        lms = ragged_batch(seed, L, big=[(3, 200)])
        b, m = matcher.ComputeDistinctiveDescriptors(lms)
        rb, rm = distinctive_descriptors_fast(lms)
        assert np.array_equal(b, rb) and np.array_equal(m, rm), (seed, L)


def test_device_entry_point_on_a_caller_stream(matcher):
    ex = matcher._ex
    s = hipmem.Stream()
    for seed, L in ((30, 3000), (31, 11), (32, 9000), (33, 0)):
        lms = ragged_batch(seed, L, big=[(1, 129), (L - 1, 70)] if L > 1 else [])
        off, desc = csr(lms)
        rb, rm = distinctive_descriptors_fast(lms)
        d_off, d_desc = hipmem.DevBuf.from_numpy(off), hipmem.DevBuf.from_numpy(desc)
        d_b, d_m = hipmem.DevBuf(4 * max(L, 1)), hipmem.DevBuf(4 * max(L, 1))
        d_b.fill(0x55); d_m.fill(0x55)
        ex.landmark_best_descriptors_device(d_off.ptr, L, d_desc.ptr, d_b.ptr, d_m.ptr, stream=s.ptr)
        s.synchronize()
        b, m = d_b.to_numpy(np.int32, L), d_m.to_numpy(np.int32, L)
        assert np.array_equal(b, rb) and np.array_equal(m, rm), (seed, L)
        if L == 0:
            assert d_b.to_numpy(np.int32, 1)[0] == 0x55555555            # nothing written for an empty batch
    # the handle's own stream (stream = 0)
    lms = ragged_batch(34, 500, big=[(2, 100)])
    off, desc = csr(lms)
    d_off, d_desc = hipmem.DevBuf.from_numpy(off), hipmem.DevBuf.from_numpy(desc)
    d_b, d_m = hipmem.DevBuf(4 * 500), hipmem.DevBuf(4 * 500)
    ex.landmark_best_descriptors_device(d_off.ptr, 500, d_desc.ptr, d_b.ptr, d_m.ptr)
    ex.synchronize()
    rb, rm = distinctive_descriptors_fast(lms)
    assert np.array_equal(d_b.to_numpy(np.int32, 500), rb) and np.array_equal(d_m.to_numpy(np.int32, 500), rm)


def test_device_entry_point_refuses_misaligned_descriptors(matcher):
    from hyslam_amd import _native as N
    ex = matcher._ex
    d_off, d_desc = hipmem.DevBuf(16), hipmem.DevBuf(64)
    d_b, d_m = hipmem.DevBuf(16), hipmem.DevBuf(16)
    assert ex._lib.hs_landmark_best_descriptors_device(ex._h, d_off.ptr, d_desc.ptr + 4, 1, d_b.ptr, d_m.ptr, None) == N.HS_ERR_INVALID


def _build_adaptor():
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_landmark_adaptor.cpp"),
                           "-o", EXE, "-L" + os.path.join(ROOT, "hyslam_amd"), "-lhyslam_amd", "-Wl,-rpath," + os.path.join(ROOT, "hyslam_amd")])


def test_cpp_adaptor(tmp_path):
    lms = ragged_batch(40, 3000, big=[(0, 66), (1500, 400)]) + [KNOWN[k][0] for k in sorted(KNOWN)]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.int32(len(lms)).tobytes())
        for d in lms:
            f.write(np.int32(len(d)).tobytes() + np.ascontiguousarray(d, np.uint8).tobytes())
    _build_adaptor()
    r = subprocess.run([EXE, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"LANDMARK ADAPTOR OK" in r.stdout, r.stdout + r.stderr
    out = np.fromfile(tmp_path / "out.bin", np.int32).reshape(4, len(lms))
    rb, rm = distinctive_descriptors_fast(lms)
    assert np.array_equal(out[0], rb) and np.array_equal(out[1], rm)
    assert np.array_equal(out[2], rb) and np.array_equal(out[3], rm)
