"""numpy float32 restatement of the contracts of as_disp_edge_check and as_disp_speckle as include/adaptive_stereo_hip.h words them,
one numpy operation per rounding, and the seeded cases and patterns the CPU and GPU tests share.  Written from the header, not
from csrc/disp_filter.hip: tests/test_disp_filter_ref_cpu.py pins it against a scene whose answer is known by counting and
against scipy.ndimage.label, tests/test_gpu_disp_filter.py holds the kernels to it bit for bit.

`wrong=` turns one rule into a plausible mistake (WRONG); the CPU test shows that the cases tell each of them from the contract."""
import numpy as np

F = np.float32
QNAN_BITS = 0x7FC00000
QNAN = np.array([QNAN_BITS], dtype=np.uint32).view(F)[0]
CODES = 7                      # 0 keep, 1-3 as as_lr_check, 4 bad input, 5 discontinuity, 6 speckle
DF_SPAN = 256                  # columns a workgroup of csrc/disp_filter.hip covers in one row
DF_ROWS = 4                    # rows of a workgroup's tile
DF_WAVE = 64                   # consecutive pixels of a row in one wave

WRONG = ("eight_connected", "strict_edge", "strict_join", "tol_from_neighbour", "unusable_not_skipped", "labels_leak")

# (B, H, W): one pixel, one row, one column, the wave's width and its neighbours, the span and its neighbours, heights on
# either side of one and two tiles, and the product's width at two pixels less than a tile's height
SHAPES = [(1, 1, 1), (1, 1, 70), (1, 9, 1), (2, 5, 63), (2, 3, 64), (1, 6, 65), (1, 3, DF_SPAN - 1), (1, 4, DF_SPAN), (1, 5, DF_SPAN + 1),
          (2, 2, 1242)]
TOLS = [(1.0, 0.0), (0.5, 0.0625)]                                   # (tol_abs, tol_rel); 0.0625 * d is exact
SPECKLES = [(1.0, 3), (0.25, 40)]                                    # (max_diff, max_size)


def bits(a):
  return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def usable(disp, code_in=None):
  """float32 [B,1,H,W] (and uint8 code_in of that shape or None) -> bool: as_lr_check's step 1 on top of the incoming code"""
  with np.errstate(invalid="ignore"):
    ok = (disp >= 0) & ~np.isposinf(disp)
  return ok if code_in is None else ok & (np.asarray(code_in) == 0)


def _shifted(a, dy, dx, fill):
  """b[y, x] = a[y + dy, x + dx] over the last two axes, `fill` outside the image"""
  H, W = a.shape[-2:]
  out = np.full_like(a, fill)
  ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
  xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
  out[..., yd, xd] = a[..., ys, xs]
  return out


def _counts(code):
  B = code.shape[0]
  flat = code.reshape(B, -1)
  return np.stack([(flat == c).sum(axis=1) for c in range(CODES)], axis=1).astype(np.int32)


# ------------------------------------------------------------------------------------------------------ as_disp_edge_check
def edge_check(disp, code_in=None, tol_abs=1.0, tol_rel=0.0, wrong=None):
  """-> dict of code (uint8), valid, jump (float32), all [B,1,H,W], and counts int32 [B,7]"""
  d = np.ascontiguousarray(disp, dtype=F)
  assert d.ndim == 4 and d.shape[1] == 1
  us = usable(d, code_in)
  with np.errstate(all="ignore"):
    rel = F(tol_rel) * d
    tol = np.fmax(F(tol_abs), rel)                                   # fmaxf: a NaN product leaves tol_abs
    assert tol.dtype == F
    jump = np.zeros_like(d)
    over = np.zeros(d.shape, dtype=bool)
    steps = [(0, -1), (0, 1), (-1, 0), (1, 0)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if wrong == "eight_connected" else [])
    for dy, dx in steps:
      dq = _shifted(d, dy, dx, F(np.nan))
      use = _shifted(us, dy, dx, False)
      if wrong == "unusable_not_skipped":
        use = _shifted(np.ones_like(us), dy, dx, False)
      e = np.abs(d - dq)
      assert e.dtype == F
      t = _shifted(tol, dy, dx, F(0)) if wrong == "tol_from_neighbour" else tol
      jump = np.where(use, np.fmax(jump, e), jump)
      over |= use & ((e >= t) if wrong == "strict_edge" else (e > t))
  cin = np.zeros(d.shape, dtype=np.uint8) if code_in is None else np.asarray(code_in, dtype=np.uint8)
  code = np.where(cin != 0, cin, np.where(~us, 4, np.where(over, 5, 0))).astype(np.uint8)
  jump = np.where(us, jump, QNAN).astype(F)
  return dict(code=code, valid=(code == 0).astype(F), jump=jump, counts=_counts(code))


# ------------------------------------------------------------------------------------------------------ as_disp_speckle
def _components(d, us, max_diff, wrong):
  """d float32 [H,W], us bool [H,W] -> int64 [H*W]: the smallest index of every usable pixel's component (itself elsewhere)"""
  H, W = d.shape
  idx = np.arange(H * W).reshape(H, W)
  ps, qs = [], []
  steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if wrong == "eight_connected" else [])
  with np.errstate(all="ignore"):
    for dy, dx in steps:
      dq = _shifted(d, dy, dx, F(np.nan))
      e = np.abs(d - dq)                                             # one subtraction; |a - b| and |b - a| are the same bits
      assert e.dtype == F
      near = (e < F(max_diff)) if wrong == "strict_join" else (e <= F(max_diff))
      joined = us & _shifted(us, dy, dx, False) & near
      ps.append(idx[joined])
      qs.append(_shifted(idx, dy, dx, -1)[joined])
  p, q = np.concatenate(ps), np.concatenate(qs)
  lab = np.arange(H * W)
  while True:                                                        # hook the larger label under the smaller, then jump
    before = lab.copy()
    lp, lq = lab[p], lab[q]
    np.minimum.at(lab, lp, lq)
    np.minimum.at(lab, lq, lp)
    np.minimum.at(lab, p, lab[q])
    np.minimum.at(lab, q, lab[p])
    lab = lab[lab]
    if np.array_equal(lab, before):
      return lab


def speckle(disp, code_in=None, max_diff=1.0, max_size=200, wrong=None):
  """-> dict of label, size (int32), code (uint8), valid (float32), all [B,1,H,W], and counts int32 [B,7]"""
  d = np.ascontiguousarray(disp, dtype=F)
  assert d.ndim == 4 and d.shape[1] == 1
  B, _, H, W = d.shape
  us = usable(d, code_in)
  if wrong == "labels_leak":                                         # the batch as one tall image
    lab = _components(d.reshape(B * H, W), us.reshape(B * H, W), max_diff, wrong).reshape(B, H * W)
    lab = lab - (np.arange(B) * H * W)[:, None]
  else:
    lab = np.stack([_components(d[b, 0], us[b, 0], max_diff, wrong) for b in range(B)])
  flat_us = us.reshape(B, H * W)
  size = np.zeros((B, H * W), dtype=np.int64)
  for b in range(B):
    roots, inverse, count = np.unique(lab[b][flat_us[b]], return_inverse=True, return_counts=True)
    size[b][flat_us[b]] = count[inverse]
  label = np.where(flat_us, lab, -1).astype(np.int32).reshape(d.shape)
  size = size.astype(np.int32).reshape(d.shape)
  cin = np.zeros(d.shape, dtype=np.uint8) if code_in is None else np.asarray(code_in, dtype=np.uint8)
  code = np.where(cin != 0, cin, np.where(~us, 4, np.where(size <= max_size, 6, 0))).astype(np.uint8)
  return dict(label=label, size=size, code=code, valid=(code == 0).astype(F), counts=_counts(code))


def disparity_filter(disp, code_in=None, tol_abs=1.0, tol_rel=0.0, max_diff=1.0, max_size=200):
  """DisparityFilter.__call__: the edge check, then the speckle pass on what it kept -> (edges, speckles)"""
  e = edge_check(disp, code_in, tol_abs, tol_rel)
  return e, speckle(disp, e["code"], max_diff, max_size)


# ------------------------------------------------------------------------------------------------------ cases
def random_case(shape, seed=0, bad=0.05, coded=0.1):
  """(disp float32, code_in uint8), both [B,1,H,W]: plateaus of a few levels under noise of about the tolerance, so that
  neighbours fall on both sides of every rule, bad values (NaN, +inf, -inf, negative, -0.0) and incoming codes 1..4 sprinkled in"""
  B, H, W = shape
  rng = np.random.default_rng(3000 * seed + 7 * W + 3 * H + B)
  disp = np.zeros((B, 1, H, W), dtype=F)
  for b in range(B):
    disp[b] = F(rng.integers(2, 30))
    for _ in range(4):
      y0, x0 = rng.integers(0, H), rng.integers(0, W)
      disp[b, 0, y0:y0 + 1 + rng.integers(0, max(1, H // 2) + 1), x0:x0 + 1 + rng.integers(0, max(1, W // 3) + 1)] = F(rng.integers(2, 30))
  kind = rng.integers(0, 3, size=disp.shape)
  noise = np.where(kind == 0, 0.0, np.where(kind == 1, np.round(rng.uniform(-1.5, 1.5, size=disp.shape) * 4) / 4,
                                            rng.uniform(-0.7, 0.7, size=disp.shape)))
  disp = np.maximum(disp + noise.astype(F), F(0)).astype(F)
  flat = disp.reshape(-1)
  spots = np.flatnonzero(rng.random(flat.size) < bad)
  flat[spots] = np.array([np.nan, np.inf, -np.inf, -1.5, -0.0], dtype=F)[np.arange(spots.size) % 5]
  code_in = np.where(rng.random(disp.shape) < coded, rng.integers(1, 5, size=disp.shape), 0).astype(np.uint8)
  return disp, code_in


def _holes(shape, keep):
  """12.5 where keep, NaN elsewhere: the pattern alone decides the components"""
  B, H, W = shape
  return np.where(np.broadcast_to(keep, (B, 1, H, W)), F(12.5), F(np.nan)).astype(F)


def checkerboard(shape):
  """every usable pixel a component of its own: the most components, and nothing to join"""
  y, x = np.indices(shape[1:])
  return _holes(shape, (y + x) % 2 == 0)


def comb(shape):
  """teeth in every other column that meet only in the last row: the smallest index wins late, across every tile"""
  y, x = np.indices(shape[1:])
  return _holes(shape, (x % 2 == 0) | (y == shape[1] - 1))


def serpentine(shape):
  """a one-pixel-wide path through every other row, turning at alternate ends: the longest chain"""
  H, W = shape[1:]
  y, x = np.indices((H, W))
  turn = np.where((y // 2) % 2 == 0, W - 1, 0)
  return _holes(shape, (y % 2 == 0) | (x == turn))


def spiral(shape):
  """a square spiral of one-pixel arms two pixels apart, from the outer corner inwards"""
  H, W = shape[1:]
  keep = np.zeros((H, W), dtype=bool)
  keep[0, 0] = True
  y = x = k = turns = 0
  while turns < 2:                                                   # walk on while the cell ahead is free and the one behind it too
    dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[k]
    ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
    if 0 <= ny < H and 0 <= nx < W and not keep[ny, nx] and not (0 <= ay < H and 0 <= ax < W and keep[ay, ax]):
      y, x, turns = ny, nx, 0
      keep[y, x] = True
    else:
      k, turns = (k + 1) % 4, turns + 1
  return _holes(shape, keep)


def u_shape(shape):
  """two arms in the first and the last column, joined only by the last row: with W > DF_SPAN and H > DF_ROWS the arms lie in
  different workgroup tiles and the smaller label must cross to the other arm through the bottom"""
  H, W = shape[1:]
  y, x = np.indices((H, W))
  return _holes(shape, (x == 0) | (x == W - 1) | (y == H - 1))


def full(shape):
  B, H, W = shape
  return np.full((B, 1, H, W), F(12.5), dtype=F)


PATTERNS = dict(checkerboard=checkerboard, comb=comb, serpentine=serpentine, spiral=spiral, u_shape=u_shape, full=full)


def tile_steps(shape):
  """a disparity that steps by 3 at every wave boundary in x and at every tile boundary in y and is flat inside: with tol 1 the
  edge check must flag exactly the pixels on either side of a boundary, each from a neighbour another wave or workgroup holds"""
  B, H, W = shape
  y, x = np.indices((H, W))
  level = 3 * (y // DF_ROWS) + 3 * (x // DF_WAVE) + 5
  return np.broadcast_to(level.astype(F), (B, 1, H, W)).copy()


# the analytic scene of the CPU test
SCENE = dict(H=24, W=40, BG=3.0, rect=(6, 18, 10, 26, 12.0), island=(1, 6, 30, 35, 7.0), pixel=(20, 3, 9.0))


def analytic_scene():
  s = SCENE
  d = np.full((1, 1, s["H"], s["W"]), s["BG"], dtype=F)
  for y0, y1, x0, x1, v in (s["rect"], s["island"]):
    d[0, 0, y0:y1, x0:x1] = v
  y, x, v = s["pixel"]
  d[0, 0, y, x] = v
  return d


def planted_case():
  """(disp [1,1,H,W], code_in, {name: (y, x)}): every plant is a short horizontal run inside a map of NaN, one plant a row two rows
  apart, so that nothing else decides its outcome.  The named pixel is the run's FIRST."""
  up, dn = F(np.inf), F(-np.inf)
  rows = [
    ("e_below", [2.0, np.nextafter(F(3.0), dn)]),                    # e just under 1
    ("e_exact", [2.0, 3.0]),                                         # e == 1 == tol_abs == max_diff: kept, joined
    ("e_above", [2.0, np.nextafter(F(3.0), up)]),                    # e = 1 + 2^-22
    ("rel_overtakes", [16.0, 16.75]),                                # tol_rel 0.0625: tol 1.0 (and 1.046875) over tol_abs 0.5
    ("rel_one_sided", [16.0, 17.03125]),                             # e 1.03125 > tol(16) = 1.0, <= tol(17.03125) = 1.064453125
    ("neg_zero", [-0.0, 0.5]),
    ("nan", [np.nan]), ("inf", [np.inf]), ("negative", [-2.0]), ("neg_inf", [-np.inf]),
    ("hole_beside_jump", [5.0, -30.0, 50.0]),                        # the middle one is not usable: neither side sees a jump
    ("coded_beside_jump", [5.0, 50.0]),                              # the second carries code_in 1
    ("size_eq", [8.0, 8.0, 8.0]),                                    # max_size 3: rejected
    ("size_plus1", [8.0, 8.0, 8.0, 8.0]),                            # kept
  ]
  H, W = 2 * len(rows) + 1, 8
  d = np.full((1, 1, H, W), np.nan, dtype=F)
  code_in = np.zeros((1, 1, H, W), dtype=np.uint8)
  where = {}
  for i, (name, values) in enumerate(rows):
    y = 2 * i + 1
    d[0, 0, y, 2:2 + len(values)] = np.array(values, dtype=F)
    where[name] = (y, 2)
  code_in[0, 0, where["coded_beside_jump"][0], 3] = 1
  return d, code_in, where
