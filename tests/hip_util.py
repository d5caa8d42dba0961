"""Device buffers for tests that call the launch-level C ABI (v2p_stitch_launch, v2p_bgzf_inflate_launch) directly: the HIP runtime
through ctypes, no torch (initialising torch after the library has taken the device fails on the test boxes)."""
import ctypes

import numpy as np

_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
        _hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        _hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        _hip.hipFree.argtypes = [ctypes.c_void_p]
    return _hip


class DevBuf:
    """`nbytes` of device memory with `pad` zeroed bytes either side of the payload (ptr points at the payload)."""

    def __init__(self, nbytes: int, pad: int = 64, fill: int = 0):
        self.nbytes, self.pad = int(nbytes), pad
        p = ctypes.c_void_p()
        assert hip().hipMalloc(ctypes.byref(p), self.nbytes + 2 * pad + 16) == 0
        self.base = p.value
        assert hip().hipMemset(self.base, fill, self.nbytes + 2 * pad + 16) == 0
        self.ptr = self.base + pad

    @classmethod
    def of(cls, arr: np.ndarray, pad: int = 64):
        arr = np.ascontiguousarray(arr)
        b = cls(arr.nbytes, pad)
        if arr.nbytes:
            assert hip().hipMemcpy(b.ptr, arr.ctypes.data, arr.nbytes, 1) == 0
        return b

    def download(self) -> np.ndarray:
        out = np.empty(self.nbytes, dtype=np.uint8)
        assert hip().hipDeviceSynchronize() == 0
        if self.nbytes:
            assert hip().hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0
        return out

    def free(self):
        if self.base:
            hip().hipFree(self.base)
            self.base = 0


def inflate_launch(z: bytes, mb, ob, out_offset: int = 0, guard: int = 4096):
    """v2p_bgzf_inflate_launch on device buffers of the HIP runtime; d_out sits `out_offset` bytes behind a 64-byte boundary, between two
    guard regions of 0xA5, and the status words are followed by 16 spare ones of 0x5A.  ob[0] need not be 0: the bytes below it belong to
    the guard.  Returns (out[0, ob[-1]), status [n + 1], guards and spare words untouched)"""
    from vcf2prot_amd import _native as N
    n = len(mb) - 1
    first, total = int(ob[0]), int(ob[-1])
    d_in = DevBuf.of(np.frombuffer(z + bytes(1), np.uint8))
    d_off = DevBuf.of(np.concatenate([np.asarray(mb, np.uint64), np.asarray(ob, np.uint64)]))
    buf = DevBuf(total + out_offset + 2 * guard, fill=0xA5)
    d_status = DevBuf(4 * (n + 1 + 16), fill=0x5A)
    lo = guard + out_offset
    rc = N.hip_lib().v2p_bgzf_inflate_launch(None, d_in.ptr, d_off.ptr, d_off.ptr + 8 * (n + 1), n, buf.ptr + lo, d_status.ptr)
    assert rc == 0 and hip().hipDeviceSynchronize() == 0
    host = buf.download()
    words = d_status.download().view(np.uint32).copy()
    for b in (d_in, d_off, buf, d_status):
        b.free()
    guards = bool((host[:lo + first] == 0xA5).all() and (host[lo + total:] == 0xA5).all() and (words[n + 1:] == 0x5A5A5A5A).all())
    return host[lo:lo + total], words[:n + 1], guards
