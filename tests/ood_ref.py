"""Host restatement (numpy) of what csrc/ood.hip and adaptive_stereo/ood.py compute, written from the contract in
include/adaptive_stereo_hip.h, plus the seeded volumes that tests/golden/make_golden_ood.py ran the reference on.

tests/test_ood_ref_cpu.py holds this file to the reference's own outputs (tests/golden/ood_fcs.npz); tests/test_gpu_ood.py then
compares the kernel with it.
"""
import numpy as np

# (B, D, H, W): the smallest shapes at which each thing can go wrong
SHAPES = [
  (1, 3, 1, 1),        # smallest D with a mean variant; one pixel
  (1, 1, 2, 2),        # D <= 2: mean map 0, median = max - min or 0
  (2, 2, 4, 4),
  (1, 5, 3, 9),        # odd D
  (2, 12, 5, 67),      # k = 4's D; a row that ends mid-wave just past 64
  (3, 24, 7, 131),     # k = 3's D; rows of two waves and a ragged tail; three images
  (1, 64, 2, 70),      # the D limit
  (4, 12, 24, 78),     # the bench workload's own coarse volume
]
GAINS = [1.0, 50.0]


def case_name(shape, gain):
  return "b%d_d%d_h%d_w%d_g%d" % (tuple(shape) + (int(gain),))


def case_seed(shape, gain):
  B, D, H, W = shape
  return 1000003 * B + 10007 * D + 101 * H + W + 7 * int(gain)


# planted pixels: (image, flattened pixel) per kind; all in image 0 but the NaN, which sits in the LAST image of a batch of two
# or more, so that image 0's scores stay finite
PLANT_KINDS = ("all_equal", "max_twice", "ties_at_median", "signed_zeros", "signed_zeros_between")


def planted(shape):
  """{kind: (b, pixel)} of the pixels make_volume plants into a volume of this shape."""
  B, D, H, W = shape
  out = {}
  if D >= 3 and H * W >= 6:
    for i, kind in enumerate(PLANT_KINDS):
      out[kind] = (0, i)
  if B >= 2 and H * W >= 6:
    out["nan"] = (B - 1, 5)
  return out


def make_volume(shape, gain, plant=True, nan=True):
  """fp32 [B,D,H,W]: gain * standard normal values from numpy's frozen legacy generator, then the planted pixels."""
  B, D, H, W = shape
  g = np.float32(gain)
  vol = np.random.RandomState(case_seed(shape, gain)).standard_normal(shape).astype(np.float32) * g
  flat = vol.reshape(B, D, H * W)
  where = planted(shape) if plant else {}
  r = (D - 1) // 2
  for kind, (b, p) in where.items():
    if kind == "all_equal":
      flat[b, :, p] = np.float32(1.5) * g
    elif kind == "max_twice":                         # the largest value at both ends of the column
      flat[b, 0, p] = flat[b, D - 1, p] = np.abs(flat[b, :, p]).max() + g
    elif kind == "ties_at_median":                    # distinct values in descending d, then ranks r-1, r, r+1 made equal
      v = (np.arange(D, dtype=np.float32) - np.float32(D // 2)) * g
      v[max(r - 1, 0):min(r + 1, D - 1) + 1] = v[r]
      flat[b, :, p] = v[::-1]
    elif kind == "signed_zeros":
      flat[b, :, p] = np.where(np.arange(D) % 2 == 0, np.float32(0.0), np.float32(-0.0))
    elif kind == "signed_zeros_between":              # one value below, one above, zeros of both signs around the median rank
      v = np.where(np.arange(D) % 2 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
      v[0], v[D - 1] = -g, g
      flat[b, :, p] = v
    elif kind == "nan" and nan:
      flat[b, D // 2, p] = np.float32("nan")
  return vol


def checksum(vol):
  """(sum, sum of squares) in fp64 over the finite values + the count of NaNs: a fingerprint of a regenerated volume."""
  v = vol.astype(np.float64).ravel()
  ok = ~np.isnan(v)
  return np.array([v[ok].sum(), (v[ok] ** 2).sum(), float((~ok).sum())], dtype=np.float64)


# ---- the two maps ---------------------------------------------------------------------------------------------------------
def has_nan(vol):
  return np.isnan(vol).any(axis=1)


def fcs_median(vol):
  """max_d - (the element of rank (D-1)//2 in ascending order, equal values in order of d), NaN where a column holds a NaN.
  The element is found by counting, never by sorting."""
  B, D, H, W = vol.shape
  r = (D - 1) // 2
  sel = np.zeros((B, H, W), np.float32)
  found = np.zeros((B, H, W), bool)
  for i in range(D):
    before = np.zeros((B, H, W), np.int64)
    for j in range(D):
      before += (vol[:, j] < vol[:, i]) | ((vol[:, j] == vol[:, i]) & (j < i))
    hit = before == r
    sel[hit] = vol[:, i][hit]
    found |= hit
  bad = has_nan(vol)
  assert bool((found | bad).all())
  with np.errstate(invalid="ignore"):
    big = np.where(bad, np.float32(0), vol.max(axis=1))
    out = (big - sel).astype(np.float32)
  out[bad] = np.float32("nan")
  return out


def fcs_mean(vol):
  """m1 - (sum - m1 - m2) / float32(D - 2) with the fp32 sum taken in increasing d from 0 and m1, m2 the two largest values
  (the second one equal to the first when the maximum occurs twice); 0 for D <= 2; NaN where a column holds a NaN."""
  B, D, H, W = vol.shape
  s = np.zeros((B, H, W), np.float32)
  m1 = np.full((B, H, W), -np.inf, np.float32)
  m2 = np.full((B, H, W), -np.inf, np.float32)
  with np.errstate(invalid="ignore"):
    for d in range(D):
      v = vol[:, d]
      s = (s + v).astype(np.float32)
      gt1 = v > m1
      gt2 = ~gt1 & (v > m2)
      m2 = np.where(gt1, m1, np.where(gt2, v, m2))
      m1 = np.where(gt1, v, m1)
    if D > 2:
      rest = ((s - m1).astype(np.float32) - m2).astype(np.float32)
      out = (m1 - (rest / np.float32(D - 2)).astype(np.float32)).astype(np.float32)
    else:
      out = np.zeros((B, H, W), np.float32)
  out[has_nan(vol)] = np.float32("nan")
  return out


def image_scores(fmean, fmedian):
  """[B,2] fp32: float32(fp64 mean over H x W) of each map."""
  B = fmean.shape[0]
  cols = [m.reshape(B, -1).astype(np.float64).mean(axis=1) for m in (fmean, fmedian)]
  return np.stack(cols, axis=1).astype(np.float32)


def ulp_gap(a, b):
  """Distance in fp32 units in the last place (of the larger magnitude); 0 where both are NaN, inf where one is."""
  a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
  both = np.isnan(a) & np.isnan(b)
  one = np.isnan(a) ^ np.isnan(b)
  with np.errstate(invalid="ignore"):
    gap = np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))
  return np.where(both, 0.0, np.where(one, np.inf, gap))


def same_values(a, b):
  """a == b element by element, a NaN matching a NaN at the same place; the sign of a zero does not count."""
  a, b = np.asarray(a), np.asarray(b)
  return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


# ---- the sweep --------------------------------------------------------------------------------------------------------------
def precision_recall_loop(train, novel, num=100):
  """A plain double loop over cutoffs and scores: the cutoff rounded to fp32, every compare in fp32."""
  train = [np.float32(v) for v in np.asarray(train).ravel()]
  novel = [np.float32(v) for v in np.asarray(novel).ravel()]
  out = dict(cutoffs=[], tp=[], fn=[], tn=[], fp=[], precision=[], recall=[])
  for cutoff in np.linspace(float(min(novel)), float(max(novel)), num):
    c = np.float32(cutoff)
    tp = fn = tn = fp = 0
    for v in novel:
      if v <= c:
        tp += 1
      else:
        fn += 1
    for v in train:
      if v <= c:
        fp += 1
      else:
        tn += 1
    out["cutoffs"].append(c); out["tp"].append(tp); out["fn"].append(fn); out["tn"].append(tn); out["fp"].append(fp)
    out["precision"].append(float(tp) / (tp + fp) if tp + fp > 0 else 1.0)
    out["recall"].append(float(tp) / (tp + fn))
  return out
