"""A tensor a kernel writes, between sentinels: shared by the GPU tests that call the native entry points directly
(tests/test_thin_conv_gpu.py, tests/test_conv_exact_gpu.py, tests/test_head_exact_gpu.py, tests/test_blur_exact_gpu.py)."""
import torch

DEV = "cuda"
GUARD = 1024                                   # elements of sentinel in front of and behind every buffer a kernel writes
# as values: 1.5e16 (bf16 and fp32), 2.3e127 (fp64): no case produces them
SENT = {torch.bfloat16: (torch.int16, 0x5A5B), torch.float32: (torch.int32, 0x5A5B5C5D), torch.float64: (torch.int64, 0x5A5B5C5D5E5F6061)}


class Guarded:
    """A tensor a kernel writes, inside a larger buffer whose head, tail AND body hold a sentinel bit pattern: a store outside the tensor
    changes head or tail, an element the kernel never stores keeps a value no case produces. offset: the tensor starts that many ELEMENTS
    behind the 16-byte-aligned address it has at offset 0 (the head grows by as much)."""

    def __init__(self, shape, dtype, offset=0):
        self.n = 1
        for d in shape:
            self.n *= int(d)
        it, self.pattern = SENT[dtype]
        self.head = GUARD + int(offset)
        self.raw = torch.full((self.head + self.n + GUARD,), self.pattern, dtype=it, device=DEV)
        assert self.raw.data_ptr() % 16 == 0 and (GUARD * self.raw.element_size()) % 16 == 0
        self.t = self.raw[self.head:self.head + self.n].view(dtype).view(tuple(shape))

    def intact(self):
        return bool((self.raw[:self.head] == self.pattern).all()) and bool((self.raw[self.head + self.n:] == self.pattern).all())

    def untouched(self):
        """nothing at all was written: head, tail and body"""
        return bool((self.raw == self.pattern).all())

    def unwritten(self):
        """how many elements of the body still hold the sentinel"""
        return int((self.raw[self.head:self.head + self.n] == self.pattern).sum())
