"""numpy restatement of the contract of as_disp_wmedian as include/adaptive_stereo_hip.h words it, and the seeded cases the CPU and
GPU tests share.  Written from the header, not from csrc/disp_smooth.hip: the taps of the window are stacked as shifted copies of
the map, ordered by a stable argsort on the int32 key, their weights accumulated, and the first index with 2 * cum >= Wt taken.
tests/test_disp_smooth_ref_cpu.py pins it against a per-pixel loop that sorts repeated values and against cases whose answer is
known; tests/test_gpu_disp_smooth.py holds the kernel to it bit for bit.

`wrong=` turns one rule into a plausible mistake (WRONG); the CPU test shows that the cases tell each of them from the contract."""
import numpy as np

F = np.float32
COUNTS = 4                     # usable and unchanged, usable and changed, filled, still rejected
LUT_SIZE = 768
DS_SPAN = 64                   # columns of a workgroup's tile in csrc/disp_smooth.hip
DS_ROWS = 16                   # rows of that tile
MAX_RADIUS = 7
NOT_A_TAP = np.int64(1) << 40  # above every int32 key

WRONG = ("upper_median", "unusable_taps_counted", "border_replicated", "tap_colour_as_centre", "float_order", "fill_gate_on_weight")

# (B, H, W): one pixel, one row, one column, an image smaller than the largest window, one row and seven columns past one tile, two
# tiles in both directions and a remainder
SHAPES = [(1, 1, 1), (1, 1, DS_SPAN + 6), (1, DS_ROWS + 5, 1), (1, 3, 5), (1, DS_ROWS + 1, DS_SPAN + 7),
          (2, 2 * DS_ROWS + 3, 2 * DS_SPAN + 5)]
SMALL = (1, 3, 5)
ONE_TILE_PLUS = (1, DS_ROWS + 1, DS_SPAN + 7)
TWO_TILES_PLUS = (2, 2 * DS_ROWS + 3, 2 * DS_SPAN + 5)


def bits(a):
  return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def keys(a):
  return np.ascontiguousarray(a, dtype=F).view(np.int32)


def usable(disp, code_in=None):
  with np.errstate(invalid="ignore"):
    ok = (disp >= 0) & ~np.isposinf(disp)
  return ok if code_in is None else ok & (np.asarray(code_in) == 0)


def quantise(guide):
  """float32 [B,C,H,W] -> int64 of 0 .. 255: clamp (a NaN becomes 0), one product, round to nearest even"""
  g = np.ascontiguousarray(guide, dtype=F)
  with np.errstate(invalid="ignore"):
    c = np.fmin(np.fmax(g, F(0)), F(1))
    s = c * F(255)
  assert s.dtype == F
  return np.rint(s).astype(np.int64)


def weight_table(sigma_color, channels):
  """DisparitySmoother's table, in float64"""
  k = np.arange(LUT_SIZE, dtype=np.float64)
  w = np.maximum(1.0, np.round(1024.0 * np.exp(-k / (255.0 * channels * sigma_color))))
  return np.where(k <= 255 * channels, w, 0.0).astype(np.int32)


def _shifted(a, dy, dx, fill, replicate=False):
  """b[..., y, x] = a[..., y + dy, x + dx]; outside the image `fill`, or the nearest pixel when replicate"""
  H, W = a.shape[-2:]
  ys, xs = np.arange(H) + dy, np.arange(W) + dx
  inside = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
  got = a[..., np.clip(ys, 0, H - 1)[:, None], np.clip(xs, 0, W - 1)[None, :]]
  return got if replicate else np.where(inside, got, fill)


def wmedian(disp, code_in=None, guide=None, lut=None, radius=1, fill=False, min_support=1, wrong=None):
  """-> dict of out (float32 [B,1,H,W]), code (uint8 [B,1,H,W]) and counts (int32 [B,4])"""
  d = np.ascontiguousarray(disp, dtype=F)
  assert d.ndim == 4 and d.shape[1] == 1 and 1 <= radius <= MAX_RADIUS and (guide is None) == (lut is None)
  B, _, H, W = d.shape
  us = usable(d, code_in)
  key = keys(d).astype(np.int64)
  rep = wrong == "border_replicated"
  if guide is not None:
    g = quantise(guide)
    assert g.shape in ((B, 1, H, W), (B, 3, H, W))
    table = np.clip(np.asarray(lut, dtype=np.int64), 0, 65535)
    assert table.shape == (LUT_SIZE,)
  tap_keys, tap_vals, tap_w, tap_on = [], [], [], []
  for dy in range(-radius, radius + 1):
    for dx in range(-radius, radius + 1):
      on = _shifted(us, dy, dx, False, rep)
      if wrong == "unusable_taps_counted":
        on = _shifted(np.ones_like(us), dy, dx, False, rep)
      if guide is None:
        w = np.ones(d.shape, dtype=np.int64)
      else:
        gq = _shifted(g, dy, dx, 0, rep)
        centre = gq if wrong == "tap_colour_as_centre" else g
        w = table[np.abs(centre - gq).sum(axis=1, keepdims=True)]
      tap_on.append(on)
      tap_w.append(np.where(on, w, 0))
      tap_keys.append(np.where(on, _shifted(key, dy, dx, 0, rep), NOT_A_TAP))
      tap_vals.append(np.where(on, _shifted(d, dy, dx, F(0), rep), F(np.inf)))
  tap_on, tap_w, tap_keys, tap_vals = (np.stack(t) for t in (tap_on, tap_w, tap_keys, tap_vals))
  n, wt = tap_on.sum(axis=0), tap_w.sum(axis=0)
  if wrong == "float_order":                                         # `<` on the values: -0.0 and +0.0 tie and keep the tap order
    with np.errstate(invalid="ignore"):
      order = np.argsort(np.where(np.isnan(tap_vals), F(np.inf), tap_vals), axis=0, kind="stable")
  else:
    order = np.argsort(tap_keys, axis=0, kind="stable")
  cum = np.cumsum(np.take_along_axis(tap_w, order, axis=0), axis=0)
  reached = (2 * cum > wt) if wrong == "upper_median" else (2 * cum >= wt)
  first = np.argmax(reached, axis=0)[None]
  m = np.take_along_axis(np.take_along_axis(tap_keys, order, axis=0), first, axis=0)[0]
  gate = wt if wrong == "fill_gate_on_weight" else n
  selected = (wt > 0) & (us | (bool(fill) & (gate >= min_support)))    # Wt > 0: the first index reached is a tap of weight > 0
  out_key = np.where(selected, m, key).astype(np.int64)
  out = (out_key & 0xFFFFFFFF).astype(np.uint32).view(F).reshape(d.shape)
  cin = np.zeros(d.shape, dtype=np.uint8) if code_in is None else np.asarray(code_in, dtype=np.uint8)
  code = np.where(selected | us, 0, np.where(cin != 0, cin, 4)).astype(np.uint8)
  slot = np.where(us, (out_key != key).astype(np.int64), np.where(selected, 2, 3)).reshape(B, -1)
  counts = np.stack([(slot == c).sum(axis=1) for c in range(COUNTS)], axis=1).astype(np.int32)
  return dict(out=out, code=code, counts=counts)


def iterate(disp, code_in=None, guide=None, lut=None, iterations=1, **kw):
  """DisparitySmoother with iterations: every pass on the previous one's out and code; the counts are the last pass's"""
  r = dict(out=disp, code=code_in)
  for _ in range(iterations):
    r = wmedian(r["out"], r["code"], guide, lut, **kw)
  return r


def default_min_support(radius):
  return ((2 * radius + 1) ** 2 + 1) // 2


# ------------------------------------------------------------------------------------------------------ cases
def random_case(shape, seed=0, channels=3, bad=0.12, coded=0.1):
  """(disp float32 [B,1,H,W], code_in uint8 [B,1,H,W], guide float32 [B,channels,H,W], lut int32 [768]): plateaus under noise with
  salt-and-pepper; bad values (NaN, +inf, -inf, negative, -0.0, +0.0) and codes 1 .. 7 sprinkled in, holes of a few pixels; a guide
  of a few flat regions under noise with values outside [0, 1] and NaN; a table with entries on either side of the clamp and zeros"""
  B, H, W = shape
  rng = np.random.default_rng(5000 * seed + 11 * W + 5 * H + B + 100 * channels)
  disp = np.zeros((B, 1, H, W), dtype=F)
  guide = np.zeros((B, channels, H, W), dtype=F)
  for b in range(B):
    disp[b] = F(rng.integers(2, 30))
    guide[b] = rng.uniform(0.1, 0.9, size=(channels, 1, 1)).astype(F)
    for _ in range(4):
      y0, x0 = rng.integers(0, H), rng.integers(0, W)
      ys, xs = slice(y0, y0 + 1 + rng.integers(0, max(1, H // 2) + 1)), slice(x0, x0 + 1 + rng.integers(0, max(1, W // 3) + 1))
      disp[b, 0, ys, xs] = F(rng.integers(2, 30))
      guide[b, :, ys, xs] = rng.uniform(0.0, 1.0, size=(channels, 1, 1)).astype(F)
  disp = (disp + rng.uniform(-0.7, 0.7, size=disp.shape).astype(F)).astype(F)
  salt = rng.random(disp.shape) < 0.08
  disp = np.where(salt, rng.uniform(0, 60, size=disp.shape).astype(F), disp).astype(F)
  disp = np.maximum(disp, F(0))
  flat = disp.reshape(-1)
  spots = np.flatnonzero(rng.random(flat.size) < bad)
  flat[spots] = np.array([np.nan, np.inf, -np.inf, -1.5, -0.0, 0.0], dtype=F)[np.arange(spots.size) % 6]
  if H * W > 40:                                                     # a hole larger than a 3 x 3 window
    y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
    disp[:, 0, y0:y0 + 5, x0:x0 + 6] = F(np.nan)
  code_in = np.where(rng.random(disp.shape) < coded, rng.integers(1, 8, size=disp.shape), 0).astype(np.uint8)
  guide = (guide + rng.normal(0, 0.03, size=guide.shape).astype(F)).astype(F)
  odd = rng.random(guide.shape)
  guide = np.where(odd < 0.03, F(np.nan), np.where(odd < 0.06, F(-0.4), np.where(odd < 0.09, F(1.7), guide))).astype(F)
  lut = np.maximum(0, 70000 - 600 * np.arange(LUT_SIZE)).astype(np.int32)          # above 65535 up to entry 7, zero from 117 on
  lut[5] = -3                                                                      # clamps to 0
  lut[300:320] = 9
  return disp, code_in, guide, lut


def ties_case(shape, seed=0):
  """a map of a few equal levels, -0.0 and +0.0 among them, with holes: the selection among equal keys and at even counts"""
  B, H, W = shape
  rng = np.random.default_rng(77 * seed + W + 3 * H + B)
  levels = np.array([-0.0, 0.0, 1.0, 1.0, 2.0, np.nan], dtype=F)
  return levels[rng.integers(0, levels.size, size=(B, 1, H, W))]


def step_scene():
  """(disp, guide [1,1,H,W]): a disparity step whose corner coincides with the guide's edge"""
  H, W = 12, 12
  y, x = np.indices((H, W))
  fg = (y >= 5) & (x >= 5)
  disp = np.where(fg, F(20), F(4)).astype(F)[None, None]
  guide = np.where(fg, F(0.9), F(0.1)).astype(F)[None, None]
  return disp, guide, fg
