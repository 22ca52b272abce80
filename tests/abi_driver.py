"""What every driver of the C ABI in these tests shares: a context, and buffers the library reads and writes.  AbiDriver keeps them in
host memory (the emulator's 'device' is the host); GpuBuffers puts them into torch device memory on a Renderer's context: class
GpuX(GpuBuffers, AbiX).  Output buffers hold SENTINEL bytes before a call, so that what a call leaves unwritten, or writes behind its
output, shows."""
from __future__ import annotations

import ctypes as C

import numpy as np

SENTINEL = 0xA5
POISON = 0xA5A5A5A5                       # a 32-bit word of SENTINEL bytes: what an output a call never wrote still reads


class AbiDriver:
    """Owns a context of `lib` unless given one.  Buffer hooks return (object that keeps the memory alive, address[, getter of a host
    copy]); a GPU driver overrides them (GpuBuffers)."""

    def __init__(self, lib, ctx=None):
        from sage_gs import _capi
        self._capi, self.lib = _capi, lib
        self.ctx, self._own = ctx, ctx is None
        if ctx is None:
            self.ctx = C.c_void_p()
            lib.check(lib.sgs_create(0, _capi.BACKEND_HIP, C.byref(self.ctx)))

    def close(self):
        if self._own and self.ctx:
            self.lib.sgs_destroy(self.ctx)
            self.ctx = None

    def _frames(self, frames):
        a = np.ascontiguousarray(frames, np.float32)
        return a, a.ctypes.data

    def _bytes(self, n):
        a = np.full(n, SENTINEL, np.uint8)
        return a, a.ctypes.data, lambda: a

    def _i64(self, n):
        a = np.full(n, -1, np.int64)
        return a, a.ctypes.data, lambda: a

    def _sync(self):
        pass

    def _put(self, data, slack=0):
        """A buffer of SENTINEL bytes holding `data` (any array) at its start, `slack` bytes longer: (keep, address, getter)."""
        b = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        keep, ptr, get = self._bytes(len(b) + slack)
        self._fill(keep, b)
        return keep, ptr, get

    def _fill(self, keep, b):
        """Writes the uint8 array `b` at the start of the buffer `keep` that _bytes made."""
        keep[:len(b)] = b


class GpuBuffers:
    """The buffer hooks over torch device buffers, on a Renderer's context."""

    def __init__(self, renderer):
        super().__init__(renderer._lib, renderer._ctx)
        self.r = renderer

    def _frames(self, frames):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(frames, np.float32)).to(self.r.device)
        return t, t.data_ptr()

    def _bytes(self, n):
        import torch
        t = torch.full((n,), SENTINEL, dtype=torch.uint8, device=self.r.device)
        return t, t.data_ptr(), lambda: t.cpu().numpy()

    def _i64(self, n):
        import torch
        t = torch.full((n,), -1, dtype=torch.int64, device=self.r.device)
        return t, t.data_ptr(), lambda: t.cpu().numpy()

    def _sync(self):
        import torch
        torch.cuda.synchronize(self.r.device)

    def _fill(self, keep, b):
        import torch
        keep[:len(b)] = torch.from_numpy(np.array(b)).to(keep.device)
