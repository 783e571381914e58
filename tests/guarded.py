"""A caller-owned device buffer for the buffer-contract tests of the GPU suites: exactly the bytes the ABI names, between two guard
bands, everything pre-filled.  Imported by the tests the way gr_factor_cases.py is."""
import ctypes as C

import torch


class Guarded:
    """`nbytes` of device memory at a 256-byte-aligned address, pre-filled with the byte `fill`, between two guard bands of `guard`
    bytes each that hold `guard_fill` (the same byte when None).  `guard` must keep the allocator's alignment."""

    def __init__(self, label, nbytes, fill, dev, guard=1 << 16, guard_fill=None):
        self.label, self.n, self.fill, self.guard = label, int(nbytes), fill, guard
        self.gfill = fill if guard_fill is None else guard_fill
        self.raw = torch.empty((guard + self.n + guard,), dtype=torch.uint8, device=dev)
        self.raw.fill_(self.gfill)
        self.mid = self.raw[guard:guard + self.n]
        self.mid.fill_(fill)
        assert self.mid.data_ptr() % 256 == 0

    @property
    def ptr(self):
        return C.c_void_p(self.mid.data_ptr())

    def disturbed(self):
        """None, or where the first guard byte that no longer holds its fill lies (byte offset from the buffer's start)."""
        for band, base in ((self.raw[:self.guard], -self.guard), (self.raw[self.guard + self.n:], self.n)):
            bad = torch.nonzero(band != self.gfill)
            if bad.numel():
                i = int(bad[0])
                return '%s (%d bytes): guard byte at offset %d of the buffer is 0x%02x, was 0x%02x (%d guard bytes disturbed)' % (
                    self.label, self.n, base + i, int(band[i]), self.gfill, int(bad.numel()))
        return None

    def poisoned(self, itemsize):
        """Number of elements of `itemsize` bytes that still hold the fill pattern."""
        if self.n == 0:
            return 0
        return int((self.mid.cpu().numpy().reshape(-1, itemsize) == self.fill).all(axis=1).sum())

    def untouched(self):
        """Every byte of the buffer still holds the fill."""
        return bool((self.mid == self.fill).all())

    def f32(self):
        return self.mid.view(torch.float32).cpu().numpy()
