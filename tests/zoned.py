"""Device outputs between red zones, for the GPU tests that call the C ABI with their own buffers."""
import numpy as np
import torch

DEV = "cuda:0"
ZONE = 64            # elements on either side of an output


class Zoned:
    """`n` elements of `dtype` on the device between two red zones; `shift` elements move the payload off its natural alignment."""

    def __init__(self, n, dtype, fill, shift=0):
        self.n, self.lo = n, ZONE + shift
        self.fill = fill
        self.buf = torch.full((n + 2 * ZONE + shift,), fill, dtype=dtype, device=DEV)
        self.t = self.buf[self.lo:self.lo + n]

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lo * self.buf.element_size()

    def set(self, arr):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(arr)).to(DEV).view(self.buf.dtype))

    def get(self):
        b = self.buf.cpu()
        assert bool((b[:self.lo] == self.fill).all()) and bool((b[self.lo + self.n:] == self.fill).all()), "a red zone was written"
        return b[self.lo:self.lo + self.n].numpy()
