"""numpy restatement of the contract of as_rectify_map and as_rectify_pair as include/adaptive_stereo_hip.h words it: a float32
version, one numpy operation per rounding, which the kernels must match bit for bit, and a float64 version of the same formulas,
which says how far fp32 is from the mathematics.  Both take arbitrary coordinate arrays, fractional ones too.  Written from the
header, not from csrc/rectify.hip.  Also the named calibrations and the SHAPES the CPU and GPU tests share.

Self-contained on purpose (numpy only): adaptive_stereo.rectify is one of the things under test."""
import numpy as np

F = np.float32
RC_SPAN = 256                  # columns a workgroup of csrc/rectify.hip covers
RC_ROWS = 4                    # rows of a workgroup's tile
RC_PX = 4                      # pixels per lane: lane, lane + 64, lane + 128, lane + 192 of the span

# |map32 - map64| in raw pixels over the full windows of KITTI_LIKE and RATIONAL: measured on the CPU from the two references
# below (tests/test_rectify_ref_cpu.py prints it): 2.5e-4 px at KITTI_LIKE, 3.1e-4 px at KITTI_LIKE_R, 7.6e-5 px at RATIONAL; the
# largest, given x4
MAP_BOUND_MEASURED = 3.1e-4
MAP_BOUND = 4 * MAP_BOUND_MEASURED
ULP1 = float(np.finfo(F).eps)  # of an output in [0.5, 1]


def bits(a):
  return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def rodrigues(rvec):
  v = np.asarray(rvec, dtype=np.float64)
  th = np.linalg.norm(v)
  if th == 0:
    return np.eye(3)
  k = v / th
  Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
  return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * Kx.dot(Kx)


class Calib(object):
  """One raw camera and its rectified view.  K = (fx, fy, cx, cy) of the raw camera, D in OpenCV's order (padded to 8 with
  zeros), R the rectifying rotation, P = (f, cx, cy) of the rectified view and t = P[0,3], raw = (H0, W0), window = the full
  rectified image (i0, j0, H, W)."""

  def __init__(self, K, D, R, P, t, raw, window):
    self.K = tuple(float(v) for v in K)
    self.D = np.zeros(8)
    self.D[:len(D)] = D
    self.R = np.asarray(R, dtype=np.float64)
    self.P, self.t = tuple(float(v) for v in P), float(t)
    self.raw, self.window = tuple(raw), tuple(window)

  def K_matrix(self):
    fx, fy, cx, cy = self.K
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])

  def P_matrix(self):
    f, cx, cy = self.P
    return np.array([[f, 0.0, cx, self.t], [0.0, f, cy, 0.0], [0.0, 0.0, 1.0, 0.0]])

  def inverse(self):
    """fp64 inv(K_new . R)"""
    return np.linalg.inv(self.P_matrix()[:, :3].dot(self.R))

  def scaled(self, s, raw, window, t=None):
    """the same lens on a sensor and a rectified image of s times the pixels per unit angle"""
    return Calib([v * s for v in self.K], self.D, self.R, [v * s for v in self.P], self.t * s if t is None else t, raw, window)

  def constants(self, dtype):
    """(m[9], fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6) in `dtype`; fp32: each rounded once, m after the fp64 inversion"""
    return tuple(dtype(v) for v in self.inverse().reshape(-1)) , tuple(dtype(v) for v in self.K), tuple(dtype(v) for v in self.D)


KITTI_R = rodrigues((0.008, -0.012, 0.004))
KITTI_LIKE = Calib((959.791, 956.925, 696.022, 224.181), (-0.36915, 0.19687, 0.0013535, 0.00056776, -0.067707), KITTI_R,
                   (721.5377, 609.5593, 172.854), 44.857, (512, 1392), (0, 0, 375, 1242))
# its right camera: another lens, another rotation, the same rectified intrinsics
KITTI_LIKE_R = Calib((903.7596, 901.9653, 695.7519, 245.0186), (-0.3639558, 0.1788651, 0.0006029694, -0.0003922424, -0.05382460),
                     rodrigues((-0.006, 0.015, -0.003)), (721.5377, 609.5593, 172.854), -339.52, (512, 1392), (0, 0, 375, 1242))
RATIONAL = Calib((240.0, 239.0, 174.0, 56.0), (0.12, -0.05, 0.001, -0.0008, 0.01, 0.1, -0.03, 0.005), rodrigues((0.05, -0.08, 0.03)),
                 (180.0, 152.0, 43.0), 0.0, (128, 348), (0, 0, 93, 310))
# a turn of atan(4/3) = 53 degrees about y: Z = 0.025 * (u - 40) + 0.6 is zero in column 16, where X / Z is infinite and, in row
# cy = 12, Y / Z is 0 / 0; left of it the camera looks behind itself
HORIZON_R = np.array([[0.6, 0.0, 0.8], [0.0, 1.0, 0.0], [-0.8, 0.0, 0.6]])
HORIZON = Calib((50.0, 50.0, 32.0, 24.0), (-0.1, 0.01, 0.001, -0.002, 0.003), HORIZON_R, (32.0, 40.0, 12.0), 0.0, (48, 64), (0, 0, 32, 64))
# the same turn with cx = 33: in column 9 the two terms of Z cancel to a rounding residue instead of 0, the ray's slope is of the
# order of 1e7, and the polynomial overflows: infinite coordinates, and finite ones beyond 2^31 beside them
HORIZON_B = Calib((50.0, 50.0, 32.0, 24.0), (-0.1, 0.01, 0.001, -0.002, 0.003), HORIZON_R, (32.0, 33.0, 12.0), 0.0, (48, 64), (0, 0, 32, 64))
IDENTITY = Calib((1.0, 1.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), np.eye(3), (1.0, 0.0, 0.0), 0.0, (1, 1), (0, 0, 1, 1))
QUARTER = KITTI_LIKE.scaled(0.25, (128, 348), (0, 0, 93, 310))           # the small stand-in the GPU shapes use
QUARTER_R = KITTI_LIKE_R.scaled(0.25, (128, 348), (0, 0, 93, 310))
CALIBS = dict(KITTI_LIKE=KITTI_LIKE, KITTI_LIKE_R=KITTI_LIKE_R, RATIONAL=RATIONAL, HORIZON=HORIZON, HORIZON_B=HORIZON_B, IDENTITY=IDENTITY, QUARTER=QUARTER,
              QUARTER_R=QUARTER_R, EIGHTH=KITTI_LIKE.scaled(0.03125, (16, 43), (0, 0, 12, 39)))

# (id, left calibration, right calibration, B, C, (H0, W0), (i0, j0, H, W), out_of_bounds): the kernel's own constants placed:
# widths 1, 3, 5 and RC_SPAN - 1, + 0, + 1; W % 4 in {0, 1, 2, 3}; H in {1, 2, RC_ROWS + 1}; B in {1, 3}; C in {1, 3}; odd i0 and
# j0; a window that leaves the raw image on each side; a raw image smaller than the window; W0 = 1; the horizon.
# out_of_bounds: the test asserts that between 20 % and 80 % of the reference's pixels are valid, so both branches run.
SHAPES = [
  ("w1", "QUARTER", "QUARTER_R", 1, 3, (128, 348), (41, 155, 1, 1), False),
  ("w3", "QUARTER", "RATIONAL", 1, 3, (128, 348), (7, 11, 2, 3), False),
  ("w5_mono", "QUARTER", "QUARTER_R", 3, 1, (128, 348), (33, 201, RC_ROWS + 1, 5), False),
  ("span-1", "QUARTER", "QUARTER_R", 1, 3, (128, 348), (11, 21, 2, RC_SPAN - 1), False),
  ("span", "QUARTER", "QUARTER_R", 3, 3, (128, 348), (9, 27, RC_ROWS + 1, RC_SPAN), False),
  ("span+1_mono", "QUARTER", "RATIONAL", 1, 1, (128, 348), (50, 25, 1, RC_SPAN + 1), False),
  ("span-2", "RATIONAL", "QUARTER", 1, 3, (128, 348), (3, 31, RC_ROWS + 1, RC_SPAN - 2), False),
  ("left", "QUARTER", "QUARTER", 1, 3, (128, 348), (21, -51, RC_ROWS + 1, 70), True),
  ("right_wide", "QUARTER", "QUARTER", 1, 3, (128, 348), (21, 283, 2, 72), True),
  ("top_wide_mono", "QUARTER", "QUARTER", 3, 1, (128, 348), (-7, 101, 12, 64), True),
  ("bottom", "QUARTER", "QUARTER", 1, 3, (128, 348), (93, 75, 14, 67), True),
  ("raw_smaller", "EIGHTH", "EIGHTH", 1, 3, (16, 43), (-3, -5, 19, 50), True),
  ("w0_1", "IDENTITY", "IDENTITY", 1, 3, (9, 1), (-1, -1, 6, 3), True),
  ("horizon", "HORIZON", "HORIZON_B", 1, 3, (48, 64), (0, 0, 32, 64), False),
  ("horizon_mono_wide", "HORIZON_B", "HORIZON", 3, 1, (48, 64), (-3, 5, RC_ROWS + 1, 60), False),
]
SHAPE_IDS = [s[0] for s in SHAPES]


def grid(window, dtype):
  """(u, v) = ((dtype)(x + j0), (dtype)(y + i0)) of every pixel of the window, each [H,W]"""
  i0, j0, H, W = window
  return np.meshgrid((np.arange(W, dtype=np.int64) + j0).astype(dtype), (np.arange(H, dtype=np.int64) + i0).astype(dtype))


def coords(cal, raw, u, v, dtype=F):
  """-> (us, vs, valid) at rectified coordinates u, v (arrays of one shape, any values); raw = (H0, W0)"""
  T = dtype
  m, (fx, fy, cx, cy), (k1, k2, p1, p2, k3, k4, k5, k6) = cal.constants(T)
  u, v = np.asarray(u, dtype=T), np.asarray(v, dtype=T)
  one, two = T(1), T(2)
  with np.errstate(all="ignore"):
    X = (m[0] * u + m[1] * v) + m[2]
    Y = (m[3] * u + m[4] * v) + m[5]
    Z = (m[6] * u + m[7] * v) + m[8]
    xn = X / Z
    yn = Y / Z
    xx = xn * xn
    yy = yn * yn
    xy = xn * yn
    r2 = xx + yy
    num = ((k3 * r2 + k2) * r2 + k1) * r2 + one
    den = ((k6 * r2 + k5) * r2 + k4) * r2 + one
    rad = num / den
    xd = (xn * rad + (two * p1) * xy) + p2 * (r2 + two * xx)
    yd = (yn * rad + p1 * (r2 + two * yy)) + (two * p2) * xy
    us = fx * xd + cx
    vs = fy * yd + cy
    assert us.dtype == T and vs.dtype == T
    valid = (Z > 0) & (us >= 0) & (us <= T(raw[1] - 1)) & (vs >= 0) & (vs <= T(raw[0] - 1))
  return us, vs, valid


def rectify_map(cal, raw, window, dtype=F):
  u, v = grid(window, dtype)
  return coords(cal, raw, u, v, dtype)


def sample(src, us, vs, valid, fill=0.0, dtype=F):
  """src uint8 [B,H0,W0,C], coordinates [H,W] -> [B,3,H,W] in `dtype`: the contract's bilinear taps, `fill` where not valid"""
  T = dtype
  src = np.asarray(src)
  B, H0, W0, C = src.shape
  su, sv = np.where(valid, us, T(0)), np.where(valid, vs, T(0))       # the conversion to int only ever sees a valid coordinate
  fx0, fy0 = np.floor(su), np.floor(sv)
  x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
  x1, y1 = np.minimum(x0 + 1, W0 - 1), np.minimum(y0 + 1, H0 - 1)
  ax, ay = su - x0.astype(T), sv - y0.astype(T)
  s = src.astype(T)
  a, b, c, d = s[:, y0, x0], s[:, y0, x1], s[:, y1, x0], s[:, y1, x1]     # [B,H,W,C]
  ax, ay = ax[None, :, :, None], ay[None, :, :, None]
  top = (b - a) * ax + a
  bot = (d - c) * ax + c
  val = (bot - top) * ay + top
  out = val / T(255)
  assert out.dtype == T
  out = np.where(valid[None, :, :, None], out, T(fill))
  out = np.moveaxis(out, 3, 1)
  return np.ascontiguousarray(np.repeat(out, 3, axis=1) if C == 1 else out)


def rectify(cal, src, window, fill=0.0, dtype=F):
  us, vs, valid = rectify_map(cal, src.shape[1:3], window, dtype)
  return sample(src, us, vs, valid, fill, dtype)


def random_raw(B, raw, C, seed):
  """uint8 [B,H0,W0,C]: a smooth ramp plus noise, so that a shifted or swapped tap shows"""
  rng = np.random.RandomState(seed)
  H0, W0 = raw
  y, x = np.mgrid[0:H0, 0:W0]
  base = (x * 3 + y * 5)[None, :, :, None] + np.arange(C)[None, None, None, :] * 40 + np.arange(B)[:, None, None, None] * 17
  return ((base + rng.randint(0, 64, size=(B, H0, W0, C))) % 256).astype(np.uint8)


def shape_case(shape, fill=0.0):
  """the inputs and the fp32 reference's answers of one entry of SHAPES"""
  name, cl, cr, B, C, raw, window, oob = shape
  out = dict(name=name, B=B, C=C, raw=raw, window=window, oob=oob, cal=(CALIBS[cl], CALIBS[cr]), fill=fill)
  out["src"] = (random_raw(B, raw, C, 11), random_raw(B, raw, C, 12))
  out["map"] = tuple(rectify_map(c, raw, window) for c in out["cal"])
  out["dst"] = tuple(sample(s, m[0], m[1], m[2], fill) for s, m in zip(out["src"], out["map"]))
  return out
