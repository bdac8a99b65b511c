"""Host restatement (numpy) of what csrc/cv_probe.hip computes, written from the contract in include/adaptive_stereo_hip.h, plus
the cases: the seeded volumes of tests/ood_ref.py (SHAPES x GAINS, planted pixels and NaN included) and a few volumes of its own
with planted extremes for the ways a parallel arg-max can go wrong.

tests/test_cv_probe_ref_cpu.py holds this file to the reference's own picks and values (tests/golden/cv_probe.npz, written by
tests/golden/make_golden_cv_probe.py); tests/test_gpu_cv_probe.py then compares the kernel with it.
"""
import numpy as np

import ood_ref

NAN32 = np.uint32(0x7FC00000).view(np.float32)
HI, LO = 0, 1


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def _peak(D, height=100.0):
  """A column of small integers with an exact map value: sum = m1 = height, m2 = 0, mean_rest = 0, f = height."""
  v = np.zeros(D, np.float32)
  v[D // 3] = np.float32(height)
  return v


def _planted(shape, gain, plants):
  """ood_ref's unplanted seeded volume with whole columns replaced: plants = [(b, p, column)]."""
  vol = ood_ref.make_volume(shape, gain, plant=False)
  B, D, H, W = shape
  flat = vol.reshape(B, D, H * W)
  for b, p, column in plants:
    flat[b, :, p] = column
  return vol


WAVE_SHAPE = (1, 12, 9, 131)      # H*W = 1179: three trips of a 512-lane workgroup, the last one ragged


def _own_cases():
  B, D, H, W = WAVE_SHAPE
  HW = H * W
  flat_15 = np.full(D, 1.5, np.float32)                        # all equal: f = +0
  neg_zeros = np.full(D, -0.0, np.float32)                     # all -0: f = -0, which equals +0 as a number
  few = (3, 12, 5, 7)                                          # H*W = 35 < 64: most lanes hold no pixel
  cases = [
    # name, shape, gain, plants, {(b, which): p} the picks the plants force
    ("max_at_last_pixel", WAVE_SHAPE, 1.0, [(0, HW - 1, _peak(D))], {(0, HI): HW - 1}),
    ("min_in_last_lane_of_a_wave", WAVE_SHAPE, 1.0, [(0, 127, flat_15)], {(0, LO): 127}),
    # p = 70 is lane 6 of wave 1, p = 515 lane 3 of wave 0 on the second trip: the later pixel sits on the lower lane
    ("tie_across_lanes", WAVE_SHAPE, 1.0, [(0, 70, _peak(D)), (0, 515, _peak(D)), (0, 71, flat_15), (0, 516, neg_zeros)],
     {(0, HI): 70, (0, LO): 71}),
    ("tie_same_lane_two_trips", WAVE_SHAPE, 1.0, [(0, 40, _peak(D)), (0, 552, _peak(D)), (0, 41, flat_15), (0, 553, flat_15)],
     {(0, HI): 40, (0, LO): 41}),
    ("fewer_pixels_than_a_wave", few, 1.0, [(1, 34, _peak(D)), (2, 0, flat_15), (2, 34, neg_zeros)],
     {(1, HI): 34, (2, LO): 0}),
  ]
  return cases


OWN_CASES = _own_cases()
OOD_CASES = [(shape, gain) for shape in ood_ref.SHAPES for gain in ood_ref.GAINS]
CASE_NAMES = [ood_ref.case_name(s, g) for s, g in OOD_CASES] + [c[0] for c in OWN_CASES]
# the cases the reference has a map for (D > 2): what the fixture stores
STORED_NAMES = [ood_ref.case_name(s, g) for s, g in OOD_CASES if s[1] > 2] + [c[0] for c in OWN_CASES]


def make_case(name):
  """(volume [B,D,H,W] fp32, gt [B,1,H,W] fp32, forced picks {(b, which): p})."""
  for shape, gain in OOD_CASES:
    if ood_ref.case_name(shape, gain) == name:
      vol, forced = ood_ref.make_volume(shape, gain), {}
      break
  else:
    own = {c[0]: c for c in OWN_CASES}[name]
    vol, forced = _planted(own[1], own[2], own[3]), own[4]
  B, D, H, W = vol.shape
  gt = np.random.RandomState(D * 1000 + H * W).uniform(0.0, D, (B, 1, H, W)).astype(np.float32)
  return vol, gt, forced


# ---- the contract ----------------------------------------------------------------------------------------------------------------
def fmap(vol):
  """The map f [B,H,W]: as_fcs_scores' mean map (ood_ref.fcs_mean restates the same loop)."""
  return ood_ref.fcs_mean(vol)


def select(f_image):
  """(p_hi, p_lo) of one image's map: the first NaN pixel both times if there is one, else numpy's first-occurrence
  argmax / argmin (fp32 compares: -0 equals +0)."""
  flat = f_image.ravel()
  bad = np.isnan(flat)
  if bad.any():
    p = int(np.argmax(bad))
    return p, p
  return int(np.argmax(flat)), int(np.argmin(flat))


def pixel_values(column):
  """(f, m1, m2, mean_rest, d_max) of one pixel's D values: the kernel's loop, one fp32 operation at a time."""
  D = len(column)
  f32 = np.float32
  s, m1, m2, d_max = f32(0), f32(-np.inf), f32(-np.inf), -1
  for d in range(D):
    x = f32(column[d])
    s = f32(s + x)
    if x > m1:
      m2, m1, d_max = m1, x, d
    elif x > m2:
      m2 = x
  if np.isnan(column).any():
    return NAN32, NAN32, NAN32, NAN32, -1
  if D <= 2:
    return f32(0), m1, m2, NAN32, d_max
  with np.errstate(invalid="ignore", over="ignore"):
    mean_rest = f32(f32(f32(s - m1) - m2) / f32(D - 2))
    return f32(m1 - mean_rest), m1, m2, mean_rest, d_max


def profile(vol):
  """[B,D] fp32: float32(fp64 mean over the pixels of the j-th largest value); all NaN for an image that holds a NaN."""
  B, D, H, W = vol.shape
  cols = vol.reshape(B, D, H * W).astype(np.float64)
  out = np.empty((B, D), np.float32)
  for b in range(B):
    if np.isnan(cols[b]).any():
      out[b] = np.float32("nan")
    else:
      out[b] = (-np.sort(-cols[b], axis=0)).mean(axis=1).astype(np.float32)
  return out


def probe(vol, gt=None):
  """dict(pix [B,2,3] int32, vals [B,2,5] fp32, slices [B,2,D] fp32, profile [B,D] fp32, p [B,2] the flattened picks)."""
  B, D, H, W = vol.shape
  f = fmap(vol)
  flat = vol.reshape(B, D, H * W)
  pix = np.zeros((B, 2, 3), np.int32)
  vals = np.zeros((B, 2, 5), np.float32)
  slices = np.zeros((B, 2, D), np.float32)
  picks = np.zeros((B, 2), np.int64)
  for b in range(B):
    for which, p in enumerate(select(f[b])):
      column = flat[b, :, p]
      fv, m1, m2, mean_rest, d_max = pixel_values(column)
      pix[b, which] = (p // W, p % W, d_max)
      vals[b, which] = (fv, m1, m2, mean_rest, gt.reshape(B, -1)[b, p] if gt is not None else NAN32)
      slices[b, which] = column
      picks[b, which] = p
      mapped = f[b].ravel()[p]
      assert (np.isnan(fv) and np.isnan(mapped)) or fv.view(np.uint32) == mapped.view(np.uint32), "the map and the loop disagree"
  return dict(pix=pix, vals=vals, slices=slices, profile=profile(vol), p=picks)


def rounding_bound(column):
  """How far the fp32 mean_rest of one column can lie from the exact mean of everything but the two largest values: D additions
  and two subtractions, each off by at most 2^-24 of a partial sum bounded by sum |v|, divided by D - 2, plus the rounding of the
  division: (D + 2) * 2^-24 * sum |v| / (D - 2) + 2^-24 * |mean_rest|."""
  c = np.asarray(column, np.float64)
  D = len(c)
  exact = np.sort(c)[::-1][2:].mean()
  return (D + 2) * 2.0 ** -24 * np.abs(c).sum() / (D - 2) + 2.0 ** -24 * abs(exact), exact


def bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)
