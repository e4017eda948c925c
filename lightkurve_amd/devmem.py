"""Device memory of the resident classes: the per-handle free list, ``DeviceBuffer`` and the upload / pointer helpers that
device.py, cubes.py and cotrend.py share (no torch: memory and copies come from liblkhip.so itself)."""
import ctypes
import threading
import weakref

import numpy as np

from . import _capi

_vp = ctypes.c_void_p
_ip = ctypes.POINTER(ctypes.c_int64)
_dp = ctypes.POINTER(ctypes.c_double)
_i32p = ctypes.POINTER(ctypes.c_int32)


# ------------------------------------------------------------------------------------------------ device memory
class _Pool(object):
    """Free list of device allocations per handle.  ``lk_dev_free`` (hipFree) synchronises the whole device, and a pipeline
    drops an intermediate batch at every stage: a dropped buffer goes back to this list instead and is handed out again
    to the next request it fits (work on one handle is stream-ordered — include/lkhip.h "Conventions" — so a kernel still
    reading the old contents finishes before the new owner's kernels start).  ``release_device_pool()`` really frees."""

    def __init__(self, handle):
        self.handle = handle
        self.free = []                  # (capacity, ptr)
        # re-entrant: a buffer that dies in a reference cycle is finalised by the cyclic collector, which may run at any
        # allocation of this thread, also inside take() while the lock is held; give() then only appends
        self.lock = threading.RLock()

    def take(self, nbytes):
        nbytes = max(int(nbytes), 1)
        with self.lock:
            fit = [i for i, (cap, _) in enumerate(self.free) if nbytes <= cap <= 2 * nbytes + (1 << 16)]
            if fit:
                return self.free.pop(min(fit, key=lambda i: self.free[i][0]))
        cap = (nbytes + 255) & ~255
        ptr = _vp()
        _capi._check(_capi._lib.lk_dev_alloc(self.handle._h, ctypes.byref(ptr), cap))
        return cap, ptr.value

    def give(self, cap, ptr):
        with self.lock:
            self.free.append((cap, ptr))

    def release(self):
        with self.lock:
            items, self.free = self.free, []
        for _cap, ptr in items:
            _capi._lib.lk_dev_free(self.handle._h, _vp(ptr))


_POOLS = {}


def _pool(handle):
    p = _POOLS.get(handle.device)
    if p is None or p.handle is not handle:
        p = _POOLS[handle.device] = _Pool(handle)
    return p


def release_device_pool():
    """hipFree every idle buffer of the device free lists (buffers still owned by live objects are not touched)."""
    for p in list(_POOLS.values()):
        p.release()


class DeviceBuffer(object):
    """``nbytes`` of HBM owned by this object (returned to the free list when it is garbage collected)."""
    __slots__ = ("ptr", "nbytes", "capacity", "handle", "__weakref__")

    def __init__(self, handle, nbytes):
        pool = _pool(handle)
        self.capacity, self.ptr = pool.take(nbytes)
        self.nbytes = int(nbytes)
        self.handle = handle
        weakref.finalize(self, pool.give, self.capacity, self.ptr)

    def upload(self, host, stream=0):
        host = np.ascontiguousarray(host)
        if host.nbytes > self.capacity:
            raise ValueError("host array of %d bytes into a device buffer of %d" % (host.nbytes, self.capacity))
        _capi._check(_capi._lib.lk_memcpy_h2d(self.handle._h, _vp(self.ptr), _vp(host.ctypes.data), host.nbytes,
                                             _vp(stream or None)))
        return host          # (the caller keeps it alive until the stream has consumed it)

    def download(self, dtype, count, out=None, stream=0, offset_bytes=0):
        """``count`` elements of ``dtype`` starting ``offset_bytes`` into the buffer -> host array (synchronises ``stream``)."""
        dtype = np.dtype(dtype)
        count = int(count)
        if out is None:
            out = np.empty(count, dtype=dtype)
        if out.dtype != dtype or out.size != count or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous %s array of %d elements" % (dtype, count))
        if offset_bytes + count * dtype.itemsize > self.capacity:
            raise ValueError("read past the end of the device buffer")
        h = self.handle
        _capi._check(_capi._lib.lk_memcpy_d2h(h._h, _vp(out.ctypes.data), _vp(self.ptr + offset_bytes), out.nbytes,
                                             _vp(stream or None)))
        _capi._check(_capi._lib.lk_stream_synchronize(h._h, _vp(stream or None)))
        return out


def _upload(handle, host, stream, dtype=np.float64):
    host = np.ascontiguousarray(host, dtype=dtype)
    buf = DeviceBuffer(handle, host.nbytes)
    keep = buf.upload(host, stream)
    return buf, keep


def _off_ptr(n_off):
    return n_off.ctypes.data_as(_ip)


def _p(buf, offset=0):
    """``buf``'s device pointer ``offset`` bytes in, as the C ABI takes it; NULL for ``None``."""
    return _vp(buf.ptr + int(offset) if buf is not None else None)
