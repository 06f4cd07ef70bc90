"""A tensor a kernel writes, between sentinels: shared by the GPU tests that call the native entry points directly
(tests/test_thin_conv_gpu.py, tests/test_conv_exact_gpu.py)."""
import torch

DEV = "cuda"
GUARD = 1024                                   # elements of sentinel in front of and behind every buffer a kernel writes
# as values: 1.5e16 (bf16 and fp32), 2.3e127 (fp64): no case produces them
SENT = {torch.bfloat16: (torch.int16, 0x5A5B), torch.float32: (torch.int32, 0x5A5B5C5D), torch.float64: (torch.int64, 0x5A5B5C5D5E5F6061)}


class Guarded:
    """A tensor a kernel writes, inside a larger buffer whose head, tail AND body hold a sentinel bit pattern: a store outside the tensor
    changes head or tail, an element the kernel never stores keeps a value no case produces."""

    def __init__(self, shape, dtype):
        self.n = 1
        for d in shape:
            self.n *= int(d)
        it, self.pattern = SENT[dtype]
        self.raw = torch.full((2 * GUARD + self.n,), self.pattern, dtype=it, device=DEV)
        self.t = self.raw[GUARD:GUARD + self.n].view(dtype).view(tuple(shape))

    def intact(self):
        return bool((self.raw[:GUARD] == self.pattern).all()) and bool((self.raw[GUARD + self.n:] == self.pattern).all())

    def untouched(self):
        """nothing at all was written: head, tail and body"""
        return bool((self.raw == self.pattern).all())
