"""The directed draws table that enumerates a RANSAC sampler (tests/test_pnp_abi.py, tests/test_sim3_abi.py): independent of hyslam_amd."""
import itertools

import numpy as np


def randi_table(n, set_size, stride):
    """uint32 [rows, stride]: one row per sequence of randi for `set_size` draws out of n, (j0, j1, ..) with j_k < n - k in lexicographic order.  The
    word of draw k is ceil(j_k * 2^32 / avail) with avail = n - k: the smallest word that the integer reduction (word * avail) >> 32 takes to j_k."""
    rows = list(itertools.product(*[range(n - k) for k in range(set_size)]))
    t = np.zeros((len(rows), stride), np.uint32)
    for r, js in enumerate(rows):
        t[r, :set_size] = [-((-j << 32) // (n - k)) for k, j in enumerate(js)]
        assert [(int(w) * (n - k)) >> 32 for k, w in enumerate(t[r, :set_size])] == list(js)
    return t
