"""Device memory for the -m gpu tests without torch: ctypes on the HIP runtime libhyslam_amd.so itself is linked against
(the same libamdhip64 instance, already loaded by the library), so pointers can be handed to the `*_device` entry points."""
import ctypes as C

import numpy as np

_hip = None


def hip():
    global _hip
    if _hip is None:
        from hyslam_amd import _native as N
        N.lib()                                         # loads libamdhip64 as a dependency
        L = C.CDLL("libamdhip64.so.7")
        L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.hipFree.argtypes = [C.c_void_p]
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        L.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        L.hipDeviceSynchronize.argtypes = []
        L.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        L.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        L.hipStreamSynchronize.argtypes = [C.c_void_p]
        L.hipStreamDestroy.argtypes = [C.c_void_p]
        L.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        L.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        L.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        L.hipEventQuery.argtypes = [C.c_void_p]
        L.hipEventDestroy.argtypes = [C.c_void_p]
        L.hipGetLastError.argtypes = []
        _hip = L
    return _hip


def _ok(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed with hipError %d" % (what, rc))


class DevBuf:
    """a hipMalloc'ed block; `.ptr` is the integer device address"""

    def __init__(self, nbytes, zero=True):
        self.nbytes = int(max(nbytes, 16))
        p = C.c_void_p()
        _ok(hip().hipMalloc(C.byref(p), self.nbytes), "hipMalloc")
        self.ptr = p.value
        if zero:
            # hipMemset on device memory is ASYNCHRONOUS to the host and runs on the null stream; the library's streams are non-blocking, so a kernel launched
            # right after could finish BEFORE the memset and have its results zeroed (seen once in ~50 000 fuzz cases as a "mismatch" of all-zero outputs)
            _ok(hip().hipMemset(self.ptr, 0, self.nbytes), "hipMemset")
            _ok(hip().hipStreamSynchronize(None), "hipStreamSynchronize")

    @classmethod
    def from_numpy(cls, a):
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes, zero=False)
        if a.nbytes:
            _ok(hip().hipMemcpy(b.ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")
        return b

    def to_numpy(self, dtype, count=None, offset=0):
        dt = np.dtype(dtype)
        n = (self.nbytes - offset) // dt.itemsize if count is None else count
        out = np.empty(n, dt)
        _ok(hip().hipDeviceSynchronize(), "hipDeviceSynchronize")
        if out.nbytes:
            _ok(hip().hipMemcpy(out.ctypes.data, self.ptr + offset, out.nbytes, 2), "hipMemcpy D2H")
        return out

    def read_after(self, stream, dtype=np.uint8, count=None, offset=0):
        """the bytes after waiting for `stream` (a Stream or a raw handle) ALONE: no device-wide wait, a plain blocking hipMemcpy.  What another stream
        still has to write is not waited for"""
        dt = np.dtype(dtype)
        n = (self.nbytes - offset) // dt.itemsize if count is None else count
        out = np.empty(n, dt)
        _ok(hip().hipStreamSynchronize(getattr(stream, "ptr", stream)), "hipStreamSynchronize")
        if out.nbytes:
            _ok(hip().hipMemcpy(out.ctypes.data, self.ptr + offset, out.nbytes, 2), "hipMemcpy D2H")
        return out

    def fill(self, byte):
        _ok(hip().hipMemset(self.ptr, byte, self.nbytes), "hipMemset")
        _ok(hip().hipStreamSynchronize(None), "hipStreamSynchronize")

    def free(self):
        if self.ptr:
            hip().hipFree(self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Stream:
    def __init__(self, non_blocking=False):
        """non_blocking: hipStreamNonBlocking — not ordered with the NULL stream either, so work that lands there by mistake is not ordered with this one"""
        p = C.c_void_p()
        if non_blocking:
            _ok(hip().hipStreamCreateWithFlags(C.byref(p), 1), "hipStreamCreateWithFlags")
        else:
            _ok(hip().hipStreamCreate(C.byref(p)), "hipStreamCreate")
        self.ptr = p.value

    def synchronize(self):
        _ok(hip().hipStreamSynchronize(self.ptr), "hipStreamSynchronize")

    def __del__(self):
        try:
            if self.ptr:
                hip().hipStreamDestroy(self.ptr)
                self.ptr = 0
        except Exception:
            pass


class Event:
    def __init__(self):
        p = C.c_void_p()
        _ok(hip().hipEventCreate(C.byref(p)), "hipEventCreate")
        self.ptr = p.value

    def record(self, stream):
        _ok(hip().hipEventRecord(self.ptr, getattr(stream, "ptr", stream)), "hipEventRecord")

    def ready(self):
        """hipEventQuery: True once everything enqueued in front of the record has completed.  "Not ready" is a status the runtime also keeps as its
        last error: it is cleared here, or the library's next hipGetLastError() check would report it as a failure of its own launch"""
        rc = hip().hipEventQuery(self.ptr)
        hip().hipGetLastError()
        if rc not in (0, HIP_ERROR_NOT_READY):
            raise RuntimeError("hipEventQuery failed with hipError %d" % rc)
        return rc == 0

    def __del__(self):
        try:
            if self.ptr:
                hip().hipEventDestroy(self.ptr)
                self.ptr = 0
        except Exception:
            pass


HIP_ERROR_NOT_READY = 600


def memset_async(dst, byte, nbytes, stream):
    """enqueued on `stream`: the host does not wait"""
    if nbytes:
        _ok(hip().hipMemsetAsync(dst, byte, nbytes, getattr(stream, "ptr", stream)), "hipMemsetAsync")


def copy_async(dst, src, nbytes, stream):
    """device to device, enqueued on `stream` (a Stream or a raw handle): the host does not wait"""
    _ok(hip().hipMemcpyAsync(dst, src, nbytes, 3, getattr(stream, "ptr", stream)), "hipMemcpyAsync D2D")


def sync():
    _ok(hip().hipDeviceSynchronize(), "hipDeviceSynchronize")
