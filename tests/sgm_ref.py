"""The numpy restatement of the semi-global matcher's four contracts (include/adaptive_stereo_hip.h, csrc/sgm.hip): census,
matching cost and path aggregation, winner selection for both views.  Vectorised over the disparity axis; integer types throughout,
fp32 only in the grey value and in the sub-pixel division.  tests/test_sgm_ref_cpu.py holds it to things that are not itself; the
GPU tests hold the kernels to it bit for bit.

``wrong=`` names one plausible mistake (WRONG); the CPU test shows that a shared case tells the contract from each."""
import numpy as np

F = np.float32
CODES = 8                           # 0 keep, 1-6 as disp_filter_ref's table, 7 not unique
OUT_OF_VIEW_COST = 64
FAR = 1 << 20                       # stands for an absent term of a minimum
PENALTIES = ((0, 0), (3, 3), (10, 120), (0, 255))
WRONG = ("p1_from_current", "m_not_subtracted", "no_reset_at_wrap", "last_minimum", "uniqueness_le", "out_of_view_zero")
DIRECTIONS = {4: ((0, 1), (0, -1), (1, 0), (-1, 0)),
              8: ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))}      # (dy, dx)

_POPCOUNT = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)


def popcount64(a):
  a = np.ascontiguousarray(a, dtype=np.uint64)
  return _POPCOUNT[a.view(np.uint8).reshape(a.shape + (8,))].sum(axis=-1, dtype=np.int32)


# ------------------------------------------------------------------------------------------------- census
def quantise(img):
  """[B,C,H,W] fp32 -> int32 [B,H,W] in 0 .. 255: every fp32 operation rounded once, a NaN gives 0 through fmax"""
  img = np.asarray(img, dtype=F)
  assert img.ndim == 4 and img.shape[1] in (1, 3)
  with np.errstate(invalid="ignore", over="ignore"):
    if img.shape[1] == 3:
      g = (F(0.299) * img[:, 0] + F(0.587) * img[:, 1]) + F(0.114) * img[:, 2]
    else:
      g = img[:, 0]
    v = g * F(255.0) + F(0.5)
    assert v.dtype == F
    return np.floor(np.fmin(np.fmax(v, F(0.0)), F(255.0))).astype(np.int32)


def census(img):
  """uint64 [B,H,W]: bit (dy + 3) * 9 + (dx + 4) is q[clamp(y + dy)][clamp(x + dx)] < q[y][x]; bits 31 and 63 stay 0"""
  q = quantise(img)
  B, H, W = q.shape
  pad = np.pad(q, ((0, 0), (3, 3), (4, 4)), mode="edge")
  out = np.zeros((B, H, W), dtype=np.uint64)
  for dy in range(-3, 4):
    for dx in range(-4, 5):
      k = (dy + 3) * 9 + (dx + 4)
      if k == 31:
        continue
      out |= (pad[:, 3 + dy:3 + dy + H, 4 + dx:4 + dx + W] < q).astype(np.uint64) << np.uint64(k)
  return out


# ------------------------------------------------------------------------------------------------- cost and aggregation
def matching_cost(cl, cr, D, wrong=None):
  """int32 [B,H,W,D]: popcount(cl[y][x] ^ cr[y][x-d]), 64 where x - d < 0"""
  B, H, W = cl.shape
  C = np.full((B, H, W, D), 0 if wrong == "out_of_view_zero" else OUT_OF_VIEW_COST, dtype=np.int32)
  for d in range(min(D, W)):
    C[:, :, d:, d] = popcount64(cl[:, :, d:] ^ cr[:, :, :W - d])
  return C


def path_step(prev, C, P1, P2, wrong=None):
  """one step of the recurrence for any number of lines: prev, C int32 [..., D]"""
  far = np.full(prev.shape[:-1] + (1,), FAR, dtype=np.int32)
  src = C if wrong == "p1_from_current" else prev
  lo = np.concatenate([far, src[..., :-1]], axis=-1)
  hi = np.concatenate([src[..., 1:], far], axis=-1)
  m = prev.min(axis=-1, keepdims=True)
  best = np.minimum(np.minimum(prev, m + P2), np.minimum(lo, hi) + P1)
  return C + best - (0 if wrong == "m_not_subtracted" else m)


def path_costs(C, dy, dx, P1, P2, wrong=None):
  """L_r int32 [B,H,W,D] of the direction r = (dy, dx) from the matching cost C.  A vertical or diagonal path is walked as the
  kernels walk it: W lines an image, x advancing by dx per row modulo W, the recurrence reset where x has just wrapped."""
  B, H, W, D = C.shape
  out = np.empty_like(C)
  L = None
  if dy == 0:
    for x in (range(W) if dx > 0 else range(W - 1, -1, -1)):
      L = C[:, :, x] if L is None else path_step(L, C[:, :, x], P1, P2, wrong)
      out[:, :, x] = L
    return out
  c = np.arange(W)
  for t in range(H):
    y = t if dy > 0 else H - 1 - t
    xs = (c + dx * t) % W
    Cy = C[:, y, xs]                                                    # [B, lines, D]
    if L is None:
      L = Cy
    else:
      reset = np.zeros(W, dtype=bool) if dx == 0 or wrong == "no_reset_at_wrap" else (xs == 0) if dx > 0 else (xs == W - 1)
      L = np.where(reset[None, :, None], Cy, path_step(L, Cy, P1, P2, wrong))
    out[:, y, xs] = L
  return out


def aggregate(cl, cr, D, P1, P2, paths, wrong=None):
  """uint16 [B,H,W,D]: the sum of the path costs over DIRECTIONS[paths]"""
  C = matching_cost(cl, cr, D, wrong)
  S = np.zeros(C.shape, dtype=np.int32)
  for dy, dx in DIRECTIONS[paths]:
    S += path_costs(C, dy, dx, P1, P2, wrong)
  assert S.max() <= 0xFFFF
  return S.astype(np.uint16)


# ------------------------------------------------------------------------------------------------- selection
def pick(s, n, uniqueness, wrong=None):
  """the winner of columns s int32 [..., D] of which the first n [...] entries exist -> (d*, value fp32, not unique)"""
  D = s.shape[-1]
  k = np.arange(D, dtype=np.int32)
  n = np.asarray(n, dtype=np.int32)[..., None]
  exists = k < n
  masked = np.where(exists, s, np.int32(FAR))
  if wrong == "last_minimum":
    dstar = (D - 1 - np.argmin(masked[..., ::-1], axis=-1)).astype(np.int32)[..., None]
  else:
    dstar = np.argmin(masked, axis=-1).astype(np.int32)[..., None]     # numpy's arg-min is the first one
  s1 = np.take_along_axis(s, dstar, axis=-1)
  lhs, rhs = s * np.int32(100 - uniqueness), s1 * np.int32(100)
  below = (lhs <= rhs) if wrong == "uniqueness_le" else (lhs < rhs)
  ambiguous = (exists & (np.abs(k - dstar) > 1) & below).any(axis=-1)
  sm = np.take_along_axis(s, np.maximum(dstar - 1, 0), axis=-1)
  sp = np.take_along_axis(s, np.minimum(dstar + 1, n - 1), axis=-1)
  den = 2 * (sm + sp - 2 * s1)
  sub = (dstar > 0) & (dstar < n - 1) & (den > 0)
  off = (sm - sp).astype(F) / np.where(sub, den, 1).astype(F)
  value = np.where(sub, dstar.astype(F) + off, dstar.astype(F)).astype(F)
  return dstar[..., 0], value[..., 0], ambiguous


def select(S, uniqueness, fill, wrong=None, rows_at_once=None):
  """S uint16 [B,H,W,D] -> dict(disp_l, code_l, disp_r, code_r [B,1,H,W], counts int32 [B,2,8]).  The right view reads the same
  volume along its diagonal: t[d] = S(y, x+d, d) for d < min(D, W - x)."""
  B, H, W, D = S.shape
  fill = F(fill)
  out = dict(disp_l=np.empty((B, 1, H, W), F), disp_r=np.empty((B, 1, H, W), F), code_l=np.empty((B, 1, H, W), np.uint8),
             code_r=np.empty((B, 1, H, W), np.uint8))
  x = np.arange(W, dtype=np.int32)
  n_right = np.minimum(D, W - x)
  step = rows_at_once or max(1, (1 << 22) // (W * D))
  for b in range(B):
    for y0 in range(0, H, step):
      s = S[b, y0:y0 + step].astype(np.int32)
      t = np.zeros_like(s)
      for d in range(min(D, W)):
        t[:, :W - d, d] = s[:, d:, d]
      for view, (col, n) in enumerate(((s, np.full(W, D, np.int32)), (t, n_right))):
        dstar, value, ambiguous = pick(col, np.broadcast_to(n, col.shape[:-1]), uniqueness, wrong)
        code = np.where(ambiguous, 7, 0).astype(np.uint8)
        if view == 0:
          code = np.where(dstar > x, 3, code).astype(np.uint8)
        disp = np.where(code == 0, value, fill).astype(F)
        if np.isnan(fill):                                              # np.where keeps the bits; make that explicit
          disp.view(np.uint32)[code != 0] = np.array(fill).view(np.uint32)
        out["disp_" + "lr"[view]][b, 0, y0:y0 + step] = disp
        out["code_" + "lr"[view]][b, 0, y0:y0 + step] = code
  out["counts"] = np.stack([np.stack([np.bincount(out[k][b].reshape(-1), minlength=CODES)[:CODES] for k in ("code_l", "code_r")])
                            for b in range(B)]).astype(np.int32)
  return out


def sgm(left, right, D, P1=10, P2=120, paths=8, uniqueness=5, fill=np.nan):
  """the whole matcher -> (select()'s dictionary, S)"""
  S = aggregate(census(left), census(right), D, P1, P2, paths)
  return select(S, uniqueness, fill), S


# ------------------------------------------------------------------------------------------------- shared cases
def random_images(B, C, H, W, seed=0):
  """images in [0, 1] with a few values outside it, a NaN and an infinity: whatever a caller may pass"""
  rng = np.random.default_rng(seed)
  img = rng.random((B, C, H, W), dtype=F)
  flat = img.reshape(-1)
  if flat.size >= 8:
    at = rng.choice(flat.size, size=4, replace=False)
    flat[at] = np.array([np.nan, -0.25, 1.5, np.inf], dtype=F)
  return img


def random_pair(B, C, H, W, shift=2, seed=0):
  """a left image and the right one it becomes under a constant disparity `shift`, with noise: costs with structure"""
  rng = np.random.default_rng(seed)
  left = rng.random((B, C, H, W), dtype=F)
  right = np.roll(left, -shift, axis=-1)
  noisy = rng.random(left.shape) < 0.15
  right = np.where(noisy, rng.random(left.shape, dtype=F), right).astype(F)
  return left, right


RECOVERY = dict(H=24, W=64, D=16, P1=10, P2=120, uniqueness=5, background=3, foreground=12, rows=(6, 18), cols=(24, 44))


def recovery_scene(seed):
  """24 x 64, every grey level drawn independently from 0 .. 255: background of disparity 3, a rectangle (rows 6 .. 17, columns
  24 .. 43) of disparity 12 in front of it; the right view in closed form, the rectangle covering the background.
  -> left, right [1,1,H,W] fp32 (level / 255), d_true int32 [H,W], scored bool [H,W]: in view (x >= d_true) and not occluded."""
  r = RECOVERY
  H, W, bg, fg = r["H"], r["W"], r["background"], r["foreground"]
  (y0, y1), (x0, x1) = r["rows"], r["cols"]
  rng = np.random.default_rng(seed)
  left = rng.integers(0, 256, size=(H, W))
  unseen = rng.integers(0, 256, size=(H, W))                            # what the right camera sees and the left one does not
  d_true = np.full((H, W), bg, dtype=np.int32)
  d_true[y0:y1, x0:x1] = fg
  right = np.empty((H, W), dtype=np.int64)
  occluded = np.zeros((H, W), dtype=bool)
  for y in range(H):
    inside = y0 <= y < y1
    for xr in range(W):
      if inside and x0 <= xr + fg < x1:
        right[y, xr] = left[y, xr + fg]                                 # the rectangle, in front
      elif xr + bg < W and not (inside and x0 <= xr + bg < x1):
        right[y, xr] = left[y, xr + bg]                                 # background that the left view sees as well
      else:
        right[y, xr] = unseen[y, xr]
    if inside:
      for x in range(W):
        if not x0 <= x < x1 and x - bg >= 0 and x0 <= x - bg + fg < x1:
          occluded[y, x] = True                                         # background whose place in the right view the rectangle takes
  scored = (np.arange(W)[None, :] >= d_true) & ~occluded
  to_image = lambda a: (a.astype(F) / F(255.0)).astype(F)[None, None]
  return to_image(left), to_image(right), d_true, scored


def recovery_rate(disp_l, d_true, scored):
  """the share of the scored pixels whose disparity lies within 1 px of the truth (a rejected pixel, NaN, does not)"""
  with np.errstate(invalid="ignore"):
    good = np.abs(disp_l[0, 0] - d_true.astype(F)) <= F(1.0)
  return float((good & scored).sum()) / float(scored.sum())
