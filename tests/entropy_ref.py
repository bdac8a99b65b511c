"""numpy restatement of as_image_entropy's contract (include/adaptive_stereo_hip.h): integer counts, then the fp64 entropy.

Held to the reference's own utils/entropy.py by tests/test_entropy_ref_cpu.py through tests/golden/entropy.npz; the GPU tests
compare the kernel with it.  Nothing here knows how the kernel walks an image.
"""
import numpy as np

BINS = 256


def quantise(x):
  """(v int64, valid bool) of fp32 x: v = (int32)(255.0f * x), the product rounded to fp32 and truncated toward zero; a product
  that is NaN, +-inf or of magnitude >= 2^31 is invalid (v = 0 there)."""
  x = np.asarray(x, np.float32)
  with np.errstate(invalid="ignore", over="ignore"):
    p = (np.float32(255.0) * x).astype(np.float32)
    valid = np.abs(p) < np.float32(2147483648.0)             # False for NaN and inf
  v = np.trunc(np.where(valid, p, np.float32(0))).astype(np.int64)
  return v, valid


def gray_bin(v):
  """The bin of an intensity, -1 when it has none."""
  return v if 0 <= v <= 255 else -1


def grad_bin(d):
  """The bin of a horizontal difference, -1 when it has none."""
  return min((d + 255) * 256 // 510, 255) if -255 <= d <= 255 else -1


def counts(image):
  """(count_g, count_d) int64 [256] of ONE image [..., H, W]: everything in front of H, W is a stack of planes."""
  image = np.asarray(image, np.float32)
  H, W = image.shape[-2], image.shape[-1]
  v, valid = quantise(image.reshape(-1, H, W))
  g = v[valid & (v >= 0) & (v <= 255)]
  count_g = np.bincount(g, minlength=BINS).astype(np.int64)
  d = v[:, :, 1:] - v[:, :, :-1]
  both = valid[:, :, 1:] & valid[:, :, :-1]
  d = d[both & (d >= -255) & (d <= 255)]
  q = np.minimum((d + 255) * 256 // 510, 255)
  count_d = np.bincount(q, minlength=BINS).astype(np.int64)
  return count_g, count_d


def entropy64(count, n):
  """-sum over bins 0..255 in order, from 0.0, of p * log2(p) for count > 0, p = count / n, in fp64; NaN for n == 0."""
  if n == 0:
    return np.float64("nan")
  s = np.float64(0.0)
  for c in count:
    if c > 0:
      p = np.float64(c) / np.float64(n)
      s = s + p * np.log2(p)
  return -s


def scores64(image):
  """(gray, gradient) fp64 of one image [..., H, W], normalised by the plane's size."""
  image = np.asarray(image)
  H, W = image.shape[-2], image.shape[-1]
  count_g, count_d = counts(image)
  return entropy64(count_g, H * W), entropy64(count_d, H * (W - 1))


def batch(images):
  """images [B,C,H,W] or [B,H,W] -> (scores fp32 [B,2] = float32(fp64), hist uint32 [B,2,256])."""
  images = np.asarray(images, np.float32)
  sc = np.zeros((images.shape[0], 2), np.float32)
  hist = np.zeros((images.shape[0], 2, BINS), np.uint32)
  for b, im in enumerate(images):
    cg, cd = counts(im)
    hist[b, 0], hist[b, 1] = cg, cd
    H, W = im.shape[-2], im.shape[-1]
    with np.errstate(invalid="ignore"):
      sc[b] = np.float32(entropy64(cg, H * W)), np.float32(entropy64(cd, H * (W - 1)))
  return sc, hist


def ulp_gap(a, b):
  """Distance in fp32 units in the last place (of the larger magnitude); 0 where both are NaN, inf where one is."""
  a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
  both = np.isnan(a) & np.isnan(b)
  one = np.isnan(a) ^ np.isnan(b)
  with np.errstate(invalid="ignore"):
    gap = np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))
  return np.where(both, 0.0, np.where(one, np.inf, gap))


# ---- the fixture's exact cases --------------------------------------------------------------------------------------------
# The images of the reference's own unit test, recorded by tests/golden/make_golden_entropy.py under the names of its test
# methods: their bins hold 1, 1/2 or 1/4 of the pixels, so every operation of the entropy is exact.
EXACT_BITS = {"test_zero_bits_01": 0.0, "test_zero_bits_02": 0.0, "test_one_bit": 1.0, "test_two_bits": 2.0}
