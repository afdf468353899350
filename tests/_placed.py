"""Operands inside NaN-poisoned device buffers, shared by the ABI edge tests (test_gpu_gemm_edges.py,
test_gpu_gat_params.py): a margin before and after, the pitch gaps and any tail rows hold
_gemm_cases.POISON_BITS, so a read outside the operand shows as a NaN in the result and a write
outside it as a changed word."""
import ctypes

import torch

from _gemm_cases import POISON_BITS

DEV = "cuda:0"
MARGIN = 64      # floats of poison before and after an operand (a multiple of 4: keeps 16-B alignment)


def _poison(n):
    return torch.full((n,), POISON_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


class Placed:
    """[batch][rows][cols] at pitch ld and batch stride (rows + tail_rows) ld + gap inside a
    poisoned buffer, `off` floats past a 16-B aligned address."""

    def __init__(self, shape, ld, off=0, gap=0, tail_rows=0, data=None):
        self.batch, self.rows, self.cols = shape
        self.ld, self.stride = ld, (self.rows + tail_rows) * ld + gap
        self.start = MARGIN + off
        self.buf = _poison(self.start + self.batch * self.stride + MARGIN)
        ar = torch.arange
        self.idx = (self.start + ar(self.batch)[:, None, None] * self.stride + ar(self.rows)[None, :, None] * ld
                    + ar(self.cols)[None, None, :])
        if data is not None:
            self.buf[self.idx.to(DEV)] = data.to(DEV).reshape(shape).to(self.buf.dtype)

    def ptr(self, z=0):
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * (self.start + z * self.stride))

    def read(self, dtype=torch.float32):
        return self.buf.view(dtype).cpu()[self.idx]

    def outside(self):
        """(count, first (batch, row, col) position) of buffer words outside the matrix that are
        no longer the poison."""
        full = self.buf.view(torch.int32).cpu()
        keep = torch.ones(full.numel(), dtype=torch.bool)
        keep[self.idx.reshape(-1)] = False
        bad = (keep & (full != POISON_BITS)).nonzero().reshape(-1)
        if bad.numel() == 0:
            return 0, None
        o = int(bad[0]) - self.start
        z, r = divmod(o, self.stride) if o >= 0 else (-1, o)
        return int(bad.numel()), (z, r // self.ld, r % self.ld)
