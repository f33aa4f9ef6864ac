"""Guarded device buffers for the -m gpu tests (on tests/hipmem.py): every output is allocated with GUARD bytes of a pattern behind it, and every
read checks that the pattern is still there."""
import numpy as np

import hipmem

GUARD = 64
PATTERN = 0x55


def dev(a):
    """an input array on the device"""
    return hipmem.DevBuf.from_numpy(np.ascontiguousarray(a))


def out_buf(nbytes):
    """an output block filled with the pattern, guard bytes behind it"""
    b = hipmem.DevBuf(nbytes + GUARD)
    b.fill(PATTERN)
    return b


def guarded(a):
    """an in/out array with guard bytes behind it"""
    a = np.ascontiguousarray(a)
    b = out_buf(a.nbytes)
    hipmem._ok(hipmem.hip().hipMemcpy(b.ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")
    return b


def read(buf, dtype, count):
    nbytes = np.dtype(dtype).itemsize * count
    raw = buf.to_numpy(np.uint8, nbytes + GUARD)
    assert (raw[nbytes:] == PATTERN).all(), "bytes written behind the output"
    return raw[:nbytes].view(dtype).copy()
