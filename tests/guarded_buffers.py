"""What the bit-for-bit GPU suites of the per-pixel code maps share (tests/test_gpu_lr_consistency.py, test_gpu_disp_filter.py,
test_gpu_both_view.py): the sentinels, outputs between sentinel guards, and the comparison of a device tensor with a numpy array."""
import numpy as np
import torch

DEV = "cuda:0"
F = np.float32
SENTINEL = -7777.0
SENTINEL_U8 = 0xA5
SENTINEL_I32 = -7777
GUARD = 64


def dev(a):
  return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want):
  """device tensor against a numpy array of the same dtype family, bit for bit"""
  got = got.cpu().numpy()
  assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
  return np.array_equal(got.view(np.uint32), want.view(np.uint32)) if got.dtype == F else np.array_equal(got, want)


class Guarded(object):
  """`count` buffers of n elements each inside one sentinel-filled allocation, GUARD elements between and around them"""

  def __init__(self, count, n, dtype=torch.float32, sentinel=SENTINEL):
    self.n, self.count, self.sentinel = n, count, sentinel
    self.raw = torch.full((count * (n + GUARD) + GUARD,), sentinel, dtype=dtype, device=DEV)
    self.views = [self.raw[GUARD + i * (n + GUARD):GUARD + i * (n + GUARD) + n] for i in range(count)]

  def guards_intact(self):
    mask = torch.ones_like(self.raw, dtype=torch.bool)
    for i in range(self.count):
      mask[GUARD + i * (self.n + GUARD):GUARD + i * (self.n + GUARD) + self.n] = False
    return bool((self.raw[mask] == self.sentinel).all())
