"""numpy float32 restatement of the contracts of as_mirror_pair, as_flip_w, as_lr_check and as_lr_fill as
include/adaptive_stereo_hip.h words them, one numpy operation per rounding, and the seeded cases the CPU and GPU tests share.
Written from the header, not from csrc/lr_consistency.hip: tests/test_lr_consistency_ref_cpu.py pins it against a scene whose
answer is known in closed form, tests/test_gpu_lr_consistency.py holds the kernels to it bit for bit."""
import numpy as np

F = np.float32
QNAN_BITS = 0x7FC00000
QNAN = np.array([QNAN_BITS], dtype=np.uint32).view(F)[0]
CODES = 5                      # 0 consistent, 1 occluded, 2 mismatch, 3 out of view, 4 bad input
FILL_SPAN = 1024               # pixels one workgroup of as_lr_fill covers in one pass (256 lanes of 4), from the header
FILL_WAVE = 256                # pixels one wave of it covers (64 lanes of 4)

SHAPES = [(1, 1, 1), (1, 3, 5), (2, 4, 63), (2, 3, 64), (1, 2, 65), (1, 2, 257), (2, 2, 1242)]      # (B, H, W)
TOLS = [(1.0, 0.0), (0.5, 0.05)]                                                                    # (tol_abs, tol_rel)


def bits(a):
  return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------- data movement
def flip_w(a):
  return a[..., ::-1].copy()


def mirror_pair(left, right):
  return np.concatenate([left, flip_w(right)], axis=0), np.concatenate([right, flip_w(left)], axis=0)


# ---------------------------------------------------------------------------------------------------------- as_lr_check
def _one_view(own, other, left_view, tol_abs, tol_rel):
  """codes and e of one view; own, other: float32 [B,H,W] in the ordinary layout"""
  W = own.shape[-1]
  x = np.arange(W, dtype=F)[None, None, :]
  with np.errstate(all="ignore"):
    ok1 = (own >= 0) & ~np.isinf(own)                              # 1
    d = np.where(ok1, own, F(0))
    u = (x - d) if left_view else (x + d)                          # 2
    ok2 = ok1 & (~(u < 0) if left_view else ~(u > F(W - 1)))
    us = np.where(ok2, u, F(0))
    i0 = np.floor(us).astype(np.int64)                             # 3
    i1 = np.minimum(i0 + 1, W - 1)
    t = us - i0.astype(F)
    a, b = np.take_along_axis(other, i0, axis=2), np.take_along_axis(other, i1, axis=2)
    df = b - a                                                     # 4: three roundings
    pr = t * df
    sm = a + pr
    r = np.where(t == 0, a, sm)
    ok3 = ok2 & np.isfinite(r) & ~(r < 0)                          # 5
    e = np.abs(d - r)                                              # 6
    rel = F(tol_rel) * d
    tol = np.maximum(F(tol_abs), rel)
    decided = np.where(e <= tol, 0, np.where(r > d, 1, 2))         # 7
  assert e.dtype == F and tol.dtype == F and u.dtype == F and sm.dtype == F
  code = np.where(ok3, decided, np.where(ok2, 4, np.where(ok1, 3, 4))).astype(np.uint8)
  diff = np.where(code < 3, e, QNAN).astype(F)
  return code, diff


def lr_check(disp_l, disp_r, tol_abs=1.0, tol_rel=0.0, mirrored=False):
  """disp_l, disp_r: float32 [B,1,H,W].  mirrored: disp_r holds the right view's pixel x at [.., W-1-x].  Returns a dict of
  code_l, code_r (uint8), valid_l, valid_r, diff_l, diff_r (float32), all [B,1,H,W] in the ordinary layout, counts int32 [B,2,5]."""
  L = np.ascontiguousarray(disp_l, dtype=F)
  R = np.ascontiguousarray(disp_r, dtype=F)
  assert L.ndim == 4 and L.shape[1] == 1 and L.shape == R.shape
  if mirrored:
    R = flip_w(R)
  B = L.shape[0]
  out = {}
  counts = np.zeros((B, 2, CODES), dtype=np.int32)
  for v, (side, own, other) in enumerate((("l", L, R), ("r", R, L))):
    code, diff = _one_view(own[:, 0], other[:, 0], side == "l", tol_abs, tol_rel)
    out["code_" + side] = code[:, None]
    out["valid_" + side] = (code == 0).astype(F)[:, None]
    out["diff_" + side] = diff[:, None]
    for c in range(CODES):
      counts[:, v, c] = (code == c).reshape(B, -1).sum(axis=1)
  out["counts"] = counts
  return out


# ---------------------------------------------------------------------------------------------------------- as_lr_fill
def lr_fill(disp, code):
  """disp float32, code uint8, both [..., W]: the smaller of the nearest code-0 values left and right in the row"""
  disp = np.ascontiguousarray(disp, dtype=F)
  W = disp.shape[-1]
  ok = np.asarray(code) == 0
  x = np.broadcast_to(np.arange(W), disp.shape)
  li = np.maximum.accumulate(np.where(ok, x, -1), axis=-1)
  ri = np.minimum.accumulate(np.where(ok, x, W)[..., ::-1], axis=-1)[..., ::-1]
  has_l, has_r = li >= 0, ri < W
  l = np.take_along_axis(disp, np.clip(li, 0, W - 1), axis=-1)
  r = np.take_along_axis(disp, np.clip(ri, 0, W - 1), axis=-1)
  with np.errstate(invalid="ignore"):
    both = np.where(r < l, r, l)
  return np.where(ok, disp, np.where(has_l & has_r, both, np.where(has_l, l, np.where(has_r, r, F(0))))).astype(F)


# ---------------------------------------------------------------------------------------------------------- cases
def check_case(shape, seed=0):
  """(disp_l, disp_r, plants): two float32 [B,1,H,W] maps around a common per-image level, integer and fractional values mixed,
  so that all five codes occur, with the edge cases planted where the width allows.  plants: {name: (view, b, y, x)} of the
  pixels whose outcome the CPU test pins by name."""
  B, H, W = shape
  rng = np.random.default_rng(1000 * seed + 7 * W + 3 * H + B)
  maps = []
  level = rng.integers(0, max(1, W // 4) + 1, size=(B, 1, 1, 1)).astype(F)        # the same in both views: most pixels agree
  for _ in range(2):
    kind = rng.integers(0, 4, size=(B, 1, H, W))
    noise = np.where(kind == 0, 0.0, np.where(kind == 1, np.round(rng.uniform(-2, 2, size=kind.shape)),
                                              np.where(kind == 2, rng.uniform(-0.4, 0.4, size=kind.shape),
                                                       rng.uniform(-2.5, 2.5, size=kind.shape))))
    maps.append(np.maximum(level + noise.astype(F), F(0)).astype(F))
  L, R = maps
  plants = {}

  def put(name, view, b, y, x, value):
    (L if view == 0 else R)[b, 0, y, x] = value
    if name:
      plants[name] = (view, b, y, x)

  for m in (L, R):                                                 # bad inputs anywhere
    n = m.size
    spots = rng.choice(n, size=min(n, max(1, n // 40)), replace=False) if n >= 4 else []
    for i, s in enumerate(spots):
      m.reshape(-1)[s] = [np.nan, np.inf, -np.inf, -1.5, -0.0][i % 5]
  put("d0_u0", 0, 0, 0, 0, 0.0)                                    # d = 0 at x = 0: u exactly 0
  put("d0_uW1", 1, 0, 0, W - 1, 0.0)                               # d = 0 at x = W - 1 in the right view: u exactly W - 1
  if W >= 63:
    y = H - 1
    put("u0", 0, 0, y, 3, 3.0); put(None, 1, 0, y, 0, 3.0)         # u exactly 0, r = 3: consistent
    put("uW1", 1, 0, y, W - 4, 3.0); put(None, 0, 0, y, W - 1, 3.0)
    # t == 0 next to a NaN neighbour: left x = 9, d = 2 -> i0 = 7, i1 = 8 = NaN
    put("nan_neighbour", 0, 0, y, 9, 2.0); put(None, 1, 0, y, 7, 2.0); put(None, 1, 0, y, 8, np.nan)
    # e around tol = 1: the neighbour below (d 1.5, r 0.5 + ulp), exactly (d 1.5, r 0.5), above with r > d (d 0.5, r 1.5 + ulp)
    # and above with r < d (d 1.5 + ulp, r 0.5); the two fractional ones sample a flat stretch so that r is a's value
    up, dn = F(np.inf), F(-np.inf)
    for name, x, d, r in (("e_below", 14, F(1.5), np.nextafter(F(0.5), up)), ("e_exact", 20, F(1.5), F(0.5)),
                          ("e_above_occ", 26, F(0.5), np.nextafter(F(1.5), up)), ("e_above_mis", 32, np.nextafter(F(1.5), up), F(0.5))):
      put(name, 0, 0, y, x, d)
      i0 = int(np.floor(F(x) - d))
      put(None, 1, 0, y, i0, r); put(None, 1, 0, y, i0 + 1, r)
    # tol_rel * d overtakes tol_abs = 0.5 at d = 20 (tol 1.0): e = 0.75 is inside only through tol_rel
    put("rel_overtakes", 0, 0, y, 55, 20.0); put(None, 1, 0, y, 35, 20.75)
  return L, R, plants


FILL_PATTERNS = ("random", "all_valid", "all_invalid", "ends_invalid", "wave_boundaries", "pass_boundaries", "long_run",
                 "single_valid", "equal_neighbours", "signed_zero_neighbours")


def fill_case(shape, seed=0):
  """(disp float32, code uint8), both [B,1,H,W]: row i follows FILL_PATTERNS[i % len]; what a pattern needs more width for than
  the row has is clipped to the row."""
  B, H, W = shape
  rng = np.random.default_rng(2000 * seed + 7 * W + 3 * H + B)
  disp = rng.uniform(0, 50, size=(B * H, W)).astype(F)
  disp[rng.random(disp.shape) < 0.2] = F(7.25)                     # ties
  code = np.zeros((B * H, W), dtype=np.uint8)

  def kill(row, lo, hi):
    lo, hi = max(lo, 0), min(hi, W)
    if lo < hi:
      code[row, lo:hi] = rng.integers(1, CODES, size=hi - lo)

  for i in range(B * H):
    p = FILL_PATTERNS[i % len(FILL_PATTERNS)]
    if p == "random":
      bad = rng.random(W) < 0.5
      code[i, bad] = rng.integers(1, CODES, size=int(bad.sum()))
    elif p == "all_invalid":
      kill(i, 0, W)
    elif p == "ends_invalid":
      kill(i, 0, 1 + W // 5); kill(i, W - 1 - W // 7, W)
    elif p == "wave_boundaries":                                   # lanes 63|64 of either scan direction, at 1 and 4 pixels a lane
      for edge in (64, FILL_WAVE, 2 * FILL_WAVE, 3 * FILL_WAVE):
        kill(i, edge - 5, edge + 6); kill(i, W - edge - 6, W - edge + 5)
    elif p == "pass_boundaries":
      kill(i, FILL_SPAN - 9, FILL_SPAN + 7); kill(i, W - FILL_SPAN - 7, W - FILL_SPAN + 9)
    elif p == "long_run":                                          # longer than a whole wave's pixels
      kill(i, W // 8, W // 8 + FILL_WAVE + 77)
    elif p == "single_valid":
      kill(i, 0, W); code[i, (W * 2) // 3] = 0
    elif p == "equal_neighbours":
      kill(i, W // 3, W // 3 + 9)
      if W // 3 - 1 >= 0 and W // 3 + 9 < W:
        disp[i, W // 3 - 1] = disp[i, W // 3 + 9] = F(11.5)
    elif p == "signed_zero_neighbours":
      a, b = W // 4, W // 2
      kill(i, a, a + 3); kill(i, b, b + 3)
      if a - 1 >= 0 and b + 3 < W and a + 3 < b - 1:
        disp[i, a - 1], disp[i, a + 3] = F(0.0), F(-0.0)
        disp[i, b - 1], disp[i, b + 3] = F(-0.0), F(0.0)
  return disp.reshape(B, 1, H, W), code.reshape(B, 1, H, W)


# the analytic scene of the CPU test: a fronto-parallel rectangle of disparity FG over a background of disparity BG
SCENE = dict(H=8, W=64, y0=2, y1=6, x0=30, x1=45, FG=12.0, BG=3.0)


def analytic_scene():
  """(disp_l, disp_r) float32 [1,1,H,W] in closed form: the rectangle covers left columns [x0, x1) and therefore right columns
  [x0 - FG, x1 - FG); everything else shows the background."""
  s = SCENE
  L = np.full((1, 1, s["H"], s["W"]), s["BG"], dtype=F)
  R = L.copy()
  L[0, 0, s["y0"]:s["y1"], s["x0"]:s["x1"]] = s["FG"]
  R[0, 0, s["y0"]:s["y1"], s["x0"] - int(s["FG"]):s["x1"] - int(s["FG"])] = s["FG"]
  return L, R
