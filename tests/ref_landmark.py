"""Independent restatement of MapPointDBEntry::_computeDistinctiveDescriptor_ (reference: src/core/MapPointDB.cpp:128-175), written from the
reference's text in plain numpy / Python: the full float N x N distance matrix, std::sort of every row, the element at index
(size_t)(0.5*(N-1)), and the first row whose median is strictly smaller than the running best (BestMedian starts at FLT_MAX, BestIdx at 0).
Observations are in the caller's order (the reference walks a std::map<KeyFrame*, FeatureDescriptor>)."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def orb_distance(a, b):
    """ORBDistance (DescriptorDistance.cpp): Hamming distance of two 32-byte descriptors"""
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def distinctive_descriptor(descs):
    """descs: (N, 32) uint8.  Returns (BestIdx, median of that row), or (-1, -1) for N == 0 (the reference returns early)."""
    descs = np.asarray(descs, np.uint8).reshape(-1, 32)
    N = len(descs)
    if N == 0:
        return -1, -1
    D = np.zeros((N, N), np.float32)
    for i in range(N):
        D[i][i] = 0
        for j in range(i + 1, N):
            dij = np.float32(orb_distance(descs[i], descs[j]))
            D[i][j] = dij
            D[j][i] = dij
    best_median, best_idx = FLT_MAX, 0
    for i in range(N):
        v = sorted(int(x) for x in D[i])
        median = v[int(0.5 * (N - 1))]
        if median < best_median:
            best_median = median
            best_idx = i
    return best_idx, int(best_median)


def distinctive_descriptors(landmarks):
    """a list of (N_i, 32) arrays -> (best, median) int32 arrays"""
    r = [distinctive_descriptor(d) for d in landmarks]
    return np.array([a for a, _ in r], np.int32), np.array([b for _, b in r], np.int32)


def distinctive_descriptors_fast(landmarks):
    """the same answer with vectorised numpy (popcount table, np.sort, np.argmin = first minimum) — for the large random batches; the CPU tests pin
    it to distinctive_descriptor() above"""
    pop = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)
    best, med = [], []
    for d in landmarks:
        d = np.asarray(d, np.uint8).reshape(-1, 32)
        N = len(d)
        if N == 0:
            best.append(-1); med.append(-1)
            continue
        D = np.zeros((N, N), np.int32)
        for b in range(32):
            D += pop[d[:, b][:, None] ^ d[:, b][None, :]]
        m = np.sort(D, axis=1)[:, int(0.5 * (N - 1))]
        i = int(np.argmin(m))
        best.append(i); med.append(int(m[i]))
    return np.array(best, np.int32), np.array(med, np.int32)
