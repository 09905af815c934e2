"""Shared by the GPU tests that hand raw device pointers to a C entry: a device buffer between sentinel-filled guard elements, so
that a write outside the part a kernel may write is seen."""
import numpy as np
import torch

GUARD = 8
SENTINEL_F, SENTINEL_I, SENTINEL_B = np.float32(-7777.0), -7777, 0xA5


class Guarded:
    """A device buffer of float32 / int32 words (or uint8 bytes) between guard elements, all filled with a sentinel: `body` is the
    part a kernel may write."""

    def __init__(self, words, dtype):
        self.sentinel = {torch.float32: SENTINEL_F, torch.int32: SENTINEL_I, torch.uint8: SENTINEL_B}[dtype]
        self.all = torch.full((words + 2 * GUARD,), float(self.sentinel) if dtype == torch.float32 else self.sentinel, dtype=dtype, device="cuda")
        self.body = self.all[GUARD:GUARD + words]

    def ptr(self):
        return self.body.data_ptr()

    def host(self):
        got = self.all.cpu().numpy()
        assert (got[:GUARD] == self.sentinel).all() and (got[-GUARD:] == self.sentinel).all(), "a guard word was written"
        return got[GUARD:-GUARD]
