"""Host restatement (numpy) of what csrc/visualize.hip and adaptive_stereo/utils/visualization.py compute, written from the
contract in include/adaptive_stereo_hip.h, plus the seeded maps that tests/golden/make_golden_visualization.py ran the reference
on.

tests/test_visualization_ref_cpu.py holds this file to the reference's own outputs (tests/golden/visualization.npz);
tests/test_gpu_visualization.py then compares the kernels with both.
"""
import numpy as np

f32 = np.float32
MAPS = ("magma", "inferno", "hot", "jet", "gray")

# [B,1,H,W]: the smallest shapes at which the kernels can still go wrong
SHAPES = [
  (1, 1, 1, 1),        # 3 output bytes: only the peeled tail
  (1, 1, 3, 7),        # 63 bytes, not a dword multiple
  (2, 1, 37, 53),      # odd bytes per image: image 1 starts misaligned, a dword straddles two automatic ranges
  (1, 1, 67, 259),     # 17353 pixels: five workgroups' partials, 17 mapping workgroups
]
KITTI = (1, 1, 375, 1242)
R115 = 0.6 * 192       # the reference's evaluate_model.py range; a Python float, as there

# (kind, vmin, vmax, colour map): every shape runs every one of these
CONFIGS = [
  ("plain", None, None, "magma"),
  ("plain", 0, 80, "magma"),
  ("plain", 0, R115, "inferno"),
  ("plain", 0.3, 77.7, "jet"),          # float32(77.7 - 0.3) != float32(77.7) - float32(0.3)
  ("plain", None, None, "hot"),
  ("plain", None, None, "gray"),
  ("constant", None, None, "magma"),
  ("nan", 0, 80, "magma"),
  ("nan", None, None, "magma"),
  ("infs", 0, 80, "magma"),
  ("pinf", None, None, "magma"),
  ("edges80", 0, 80, "magma"),
  ("edges115", 0, R115, "inferno"),
]
MIXED = ("plain", 0, None, "magma")     # against the restatement only
# the fixture's size: the largest shape runs the configurations that need several workgroups (the automatic ranges, and the
# planted bin edges under a fixed one); the float outputs, 12 and 32 bytes a pixel, are stored for the two smallest shapes whole and for
# the batch of two under the two automatic configurations the wrappers' tests read
LARGE_CONFIGS = [CONFIGS[i] for i in (0, 8, 10, 12)]
FLOAT_CONFIGS = [CONFIGS[i] for i in (0, 8)]


def configs_for(shape):
  return LARGE_CONFIGS if shape[0] * shape[2] * shape[3] > 4000 else CONFIGS


def stores_float(shape, config):
  """Whether the fixture holds the reference's float outputs (f32__, rgba__) of this case."""
  pixels = shape[0] * shape[2] * shape[3]
  return pixels <= 400 or (pixels <= 4000 and config in FLOAT_CONFIGS)


def case_name(shape, config):
  kind, vmin, vmax, cmap = config
  rng = "auto" if vmin is None and vmax is None else "%s_%s" % (vmin, "auto" if vmax is None else "%.4g" % vmax)
  return "b%d_h%d_w%d__%s__%s__%s" % (shape[0], shape[2], shape[3], kind, rng.replace(".", "p"), cmap)


def case_seed(shape, kind):
  return 7919 * shape[0] + 101 * shape[2] + shape[3] + 13 * len(kind)


def reciprocal_biters(vmin, vmax, N=256, limit=64):
  """Values where (v - lo) * (1 / den) lands in another table bin than (v - lo) / den, found by walking the bin edges: for every
  k the 33 floats around float32(k * den / N).  Deterministic; empty for a den whose reciprocal is exact."""
  lo, den = f32(vmin), f32(float(vmax) - float(vmin))
  rcp = f32(1.0) / den
  out = []
  for k in range(1, N):
    v = f32(lo + f32(k) * den / f32(N))
    cand = [v]
    a = b = v
    for _ in range(16):
      a, b = np.nextafter(a, f32(-np.inf), dtype=f32), np.nextafter(b, f32(np.inf), dtype=f32)
      cand += [a, b]
    cand = np.array(cand, f32)
    t_div = ((cand - lo) / den * f32(N)).astype(f32)
    t_rcp = ((cand - lo) * rcp * f32(N)).astype(f32)
    hit = np.trunc(t_div) != np.trunc(t_rcp)
    out += list(cand[hit])
    if len(out) >= limit:
      break
  return np.array(out[:limit], f32)


def make_case(shape, kind):
  """fp32 [B,1,H,W] from numpy's frozen legacy generator: disparities in [0, 96 * (b + 1)) so the images of a batch have
  different ranges and some pixels exceed 80 and 115.2, then the planted values of `kind` in the LAST pixels of image 0 (as many as fit, the
  first ones first): in a batch they sit against the boundary to image 1."""
  B, _, H, W = shape
  rs = np.random.RandomState(case_seed(shape, kind))
  x = (rs.random_sample(shape) * 96.0).astype(f32)
  x *= (np.arange(B, dtype=f32) + f32(1)).reshape(B, 1, 1, 1)
  flat = x.reshape(B, H * W)
  plant = []
  if kind == "constant":
    flat[:] = f32(7.5)
  elif kind == "nan":
    plant = [f32("nan")]
  elif kind == "infs":
    plant = [f32("inf"), f32("-inf")]
  elif kind == "pinf":
    plant = [f32("inf")]
  elif kind == "edges80":
    plant = [f32(-0.0), f32(80.0), f32(80.5), f32(-0.25), np.nextafter(f32(80.0), f32(0))]
    for k in range(1, 256):
      e = f32(k * 0.3125)                                            # exactly t == k
      plant += [e, np.nextafter(e, f32(0))]                          # and the last value of bin k - 1
  elif kind == "edges115":
    plant = [f32(-0.0), f32(R115), np.nextafter(f32(R115), f32(np.inf)), f32(-1.0)] + list(reciprocal_biters(0, R115))
  elif kind != "plain":
    raise ValueError(kind)
  n = min(len(plant), H * W)
  if n:
    flat[0, H * W - n:] = np.array(plant[:n], f32)
  return x


def checksum(x):
  """(sum, sum of squares) in fp64 over the finite values + the count of non-finite ones: a fingerprint of a regenerated map."""
  v = x.astype(np.float64).ravel()
  ok = np.isfinite(v)
  return np.array([v[ok].sum(), (v[ok] ** 2).sum(), float((~ok).sum())], dtype=np.float64)


# ---- the contract -------------------------------------------------------------------------------------------------------------
def bounds(v, vmin, vmax):
  """(lo, den) fp32, each a scalar or [B,1], for v [B,HW]."""
  if vmin is not None and vmax is not None:
    return f32(float(vmin)), f32(float(vmax) - float(vmin))
  with np.errstate(invalid="ignore"):
    lo = v.min(axis=1, keepdims=True) if vmin is None else f32(float(vmin))    # numpy's min / max propagate a NaN, as torch's
    hi = v.max(axis=1, keepdims=True) if vmax is None else f32(float(vmax))
    return lo, (hi - lo).astype(f32)


def index(x, vmin=None, vmax=None, N=256, y=None, reciprocal=False):
  """int16 [B,H,W] table index of x [B,1,H,W] (or of |y - x|); N, N + 1, N + 2 = under, over, bad.  reciprocal=True is the
  WRONG arithmetic (a multiplication by 1 / den), kept to prove that a planted case tells the two apart."""
  B, _, H, W = x.shape
  v = x.reshape(B, H * W).astype(f32)
  with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
    if y is not None:
      v = np.abs(y.reshape(B, H * W).astype(f32) - v).astype(f32)
    lo, den = bounds(v, vmin, vmax)
    num = (v - lo).astype(f32)
    n = (num * (f32(1.0) / den)).astype(f32) if reciprocal else (num / den).astype(f32)
    t = (n * f32(N)).astype(f32)
    idx = np.where(np.isnan(t), N + 2, np.where(t == N, N - 1, np.where(t < 0, N, np.where(t > N, N + 1, np.trunc(t)))))
  return idx.astype(np.int16).reshape(B, H, W)


def table_u8(table):
  return (255.0 * table[:, :3]).astype(np.uint8)


def paint_u8(table, idx, order="bgr"):
  """uint8 [B,H,W,3]."""
  out = table_u8(table)[idx.astype(np.int64)]
  return np.ascontiguousarray(out[..., ::-1]) if order == "bgr" else out


def paint_f32(table, idx):
  """fp32 [B,3,H,W]: float32(table)[idx], RGB planes."""
  return np.ascontiguousarray(np.moveaxis(table.astype(f32)[idx.astype(np.int64)][..., :3], -1, 1))


def paint_rgba(table, idx):
  """float64 [B,H,W,4]: what apply_cmap returns."""
  return table[idx.astype(np.int64)]


# ---- conversions without a colour map ---------------------------------------------------------------------------------------
def saturate_u8(t):
  with np.errstate(invalid="ignore"):
    return np.where(t >= 255, 255, np.where(t > 0, np.trunc(t), 0)).astype(np.uint8)


def to_cv_rgb(img):
  """[3,H,W] -> [H,W,3] uint8 BGR."""
  return saturate_u8(np.moveaxis((f32(255.0) * img.astype(f32)).astype(f32), 0, -1)[..., ::-1])


def to_cv_gray(img):
  """[1,H,W] -> [H,W,1] uint8."""
  return saturate_u8(np.moveaxis((f32(255.0) * img.astype(f32)).astype(f32), 0, -1))


def to_cv_disp(disp, cast_uint8=True):
  """[1,H,W] -> [H,W,1]: (255.0f * d) / (float)W, two roundings."""
  W = disp.shape[2]
  t = ((f32(255.0) * disp.astype(f32)).astype(f32) / f32(W)).astype(f32)
  t = np.moveaxis(t, 0, -1)
  return saturate_u8(t) if cast_uint8 else t


CONVERSION_SHAPES = [(1, 1), (3, 7), (37, 53)]


def make_image(channels, hw, seed=0):
  """fp32 [C,H,W] in [0,1] with 0, 1, and both sides of a few k/255 edges planted (as many as fit)."""
  H, W = hw
  rs = np.random.RandomState(4242 + 17 * channels + 3 * H + W + seed)
  x = rs.random_sample((channels, H, W)).astype(f32)
  plant = [f32(1.0), f32(0.0)]
  for k in (1, 17, 128, 254):
    e = f32(k) / f32(255.0)
    plant += [e, np.nextafter(e, f32(0)), np.nextafter(e, f32(1))]
  flat = x.reshape(-1)
  n = min(len(plant), flat.size)
  flat[:n] = np.array(plant[:n], f32)
  return x


def make_disp_image(hw, seed=0):
  """fp32 [1,H,W] of disparities in [0, W)."""
  H, W = hw
  rs = np.random.RandomState(977 + 3 * H + W + seed)
  return (rs.random_sample((1, H, W)) * W * 0.999).astype(f32)


# ---- a colour map that is not matplotlib's -------------------------------------------------------------------------------------
class TenSteps(object):
  """A duck-typed colour map: N = 10 grey steps, red below, blue above, green for NaN.  Callable on an int array (table rows)
  and on floats, as a matplotlib Colormap is."""
  N = 10

  def __call__(self, v):
    v = np.asarray(v)
    out = np.zeros(v.shape + (4,), np.float64)
    out[..., 3] = 1.0
    if v.dtype.kind in "iu":
      i = v.astype(np.int64)
    else:
      with np.errstate(invalid="ignore"):
        i = np.where(np.isnan(v), 12, np.where(v < 0, 10, np.where(v > 1, 11, np.minimum(np.nan_to_num(v) * 10, 9)))).astype(np.int64)
    grey = np.clip(i, 0, 9) / 9.0
    for c in range(3):
      out[..., c] = grey
    out[i == 10] = (1, 0, 0, 1)
    out[i == 11] = (0, 0, 1, 1)
    out[i == 12] = (0, 1, 0, 1)
    return out


class TableColormap(object):
  """A colour-map object over a given [N + 3, 4] table, answering the four public calls a table is read off with."""

  def __init__(self, table):
    self.table = np.asarray(table, np.float64)
    self.N = self.table.shape[0] - 3

  def __call__(self, v):
    v = np.asarray(v)
    if v.dtype.kind in "iu":
      return self.table[v.astype(np.int64)]
    n = self.N
    with np.errstate(invalid="ignore"):
      i = np.where(np.isnan(v), n + 2, np.where(v < 0, n, np.where(v > 1, n + 1, np.minimum(np.nan_to_num(v) * n, n - 1))))
    return self.table[i.astype(np.int64)]
