"""Host restatement (numpy, float64) of what csrc/lidar.hip and adaptive_stereo/lidar.py compute, written from the contract in
include/adaptive_stereo_hip.h, plus the seeded scans and synthetic calibration files that tests/golden/make_golden_lidar.py ran
the reference's scripts/export_gt_disp.py on.

tests/test_lidar_ref_cpu.py holds this file to the reference's own outputs (tests/golden/lidar_gt.npz); tests/test_gpu_lidar.py
then compares the kernels with it.  The one deliberate difference from the reference: duplicates are resolved per pixel, where
the reference's linear index row * (W - 1) + col - 1 merges pixel (r, W-1) with pixel (r+1, 0) — only columns 0 and W-1 differ.
"""
import os

import numpy as np

F = np.float32
EMPTY = np.uint32(0xFFFFFFFF)
BASELINE = 0.54

# name: (H, W, points, seed)
SCANS = {
  "general": (75, 131, 3001, 20211),     # a row width that ends rows mid-wave; a count that is no multiple of 64, > one workgroup
  "dyadic": (24, 40, 1531, 20212),       # every q0/q2 and q1/q2 exact, most of them exactly k + 0.5 for even and odd k
}
DATES = {"general": "2011_09_26", "dyadic": "2011_09_28"}
DRIVES = {"general": "2011_09_26_drive_0001_sync", "dyadic": "2011_09_28_drive_0002_sync"}
FRAME = "0000000005"


# ---- calibration ----------------------------------------------------------------------------------------------------------
def _rot(ax, ay, az):
  cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
  Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
  Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
  Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
  return Rz.dot(Ry).dot(Rx)


def make_calibration(name):
  """The matrices of the two calibration files, float64, BEFORE they are written with %.12e (the files are the truth)."""
  H, W, _, seed = SCANS[name]
  if name == "dyadic":
    P2 = np.array([[32.0, 0, 16, 0], [0, 32, 8, 0], [0, 0, 1, 0]])
    P3 = P2.copy()
    P3[0, 3] = -8.0
    return dict(R=np.eye(3), T=np.zeros(3), R_rect_00=np.eye(3), P_rect_02=P2, P_rect_03=P3, S_rect_02=np.array([W, H], float))
  r = np.random.RandomState(seed)
  axes = np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]])            # camera x = -velodyne y, y = -z, z = x
  R = _rot(*(0.02 * (2 * r.rand(3) - 1))).dot(axes)
  T = np.array([0.013, -0.071, -1.5])                                 # scans' first 1.5 m lie BEHIND the camera: q2 < 0
  Rr = _rot(*(0.01 * (2 * r.rand(3) - 1)))
  fx, fy, cx, cy = 98.7654321, 97.1234567, 64.3, 36.9
  P2 = np.array([[fx, 0, cx, 4.53], [0, fy, cy, 0.21], [0, 0, 1, 0.0027]])
  P3 = np.array([[fx, 0, cx, -33.17], [0, fy, cy, 0.19], [0, 0, 1, 0.0031]])
  return dict(R=R, T=T, R_rect_00=Rr, P_rect_02=P2, P_rect_03=P3, S_rect_02=np.array([W, H], float))


def _row(key, values):
  return "%s: %s\n" % (key, " ".join("%.12e" % v for v in np.asarray(values, float).ravel()))


def write_calibration(calib_dir, name):
  """calib_cam_to_cam.txt and calib_velo_to_cam.txt, byte for byte the same on every run."""
  c = make_calibration(name)
  os.makedirs(calib_dir, exist_ok=True)
  with open(os.path.join(calib_dir, "calib_cam_to_cam.txt"), "w") as f:
    f.write("calib_time: 09-Jan-2012 13:57:47\n")
    f.write("rig: synthetic %s\n" % name)
    f.write(_row("corner_dist", [0.0995]))
    for key in ("S_rect_02", "R_rect_00", "P_rect_02", "P_rect_03"):
      f.write(_row(key, c[key]))
  with open(os.path.join(calib_dir, "calib_velo_to_cam.txt"), "w") as f:
    f.write("calib_time: 15-Mar-2012 11:37:16\n")
    f.write(_row("R", c["R"]))
    f.write(_row("T", c["T"]))


def compose(c):
  """{cam: 3x4 float64 velodyne -> image} from a dict of matrices as make_calibration gives (or as parsed from the files)."""
  velo2cam = np.eye(4)
  velo2cam[:3, :3] = np.asarray(c["R"]).reshape(3, 3)
  velo2cam[:3, 3] = np.asarray(c["T"]).ravel()
  rect = np.eye(4)
  rect[:3, :3] = np.asarray(c["R_rect_00"]).reshape(3, 3)
  return {cam: np.dot(np.dot(np.asarray(c["P_rect_0%d" % cam]).reshape(3, 4), rect), velo2cam) for cam in (2, 3)}


def file_calibration(name):
  """The calibration as the written files hold it: every value rounded through %.12e."""
  c = make_calibration(name)
  return {k: np.array([float("%.12e" % v) for v in np.asarray(v, float).ravel()]).reshape(np.asarray(v).shape) for k, v in c.items()}


def projections(name):
  return compose(file_calibration(name))


def bf(name):
  return BASELINE * file_calibration(name)["P_rect_02"][0, 0]


# ---- scans ----------------------------------------------------------------------------------------------------------------
def point_at(P, x, u, v):
  """(x, y, z) with the given x that P projects onto pixel (v, u) (its centre, before rounding): two linear equations in y, z."""
  A = np.array([P[0] - (u + 1.0) * P[2], P[1] - (v + 1.0) * P[2]])
  y, z = np.linalg.solve(A[:, 1:3], -(A[:, 0] * x + A[:, 3]))
  return [x, y, z]


def make_scan(name, overflow=False):
  """fp32 [N,4] in KITTI layout.  overflow: the last regular point is replaced by one at x = 0.01 alone in its pixel, whose
  128 * disp does not fit uint16 (device-only cases: the reference asserts there)."""
  H, W, N, seed = SCANS[name]
  r = np.random.RandomState(seed)
  if name == "dyadic":
    pts = []
    for z in (4.0, 8.0, 16.0):
      for k in range(16, 40):
        for m in range(0, 24):
          if r.rand() < 0.8:
            pts.append([z * (k + 0.5 - 16) / 32, z * (m + 0.5 - 8) / 32, z, r.rand()])
    pts = np.array(pts)
    off = pts[r.permutation(len(pts))[:N - len(pts)]].copy()          # the rest: the same rays a quarter pixel off the half
    off[:, 0] += off[:, 2] * 0.25 / 32
    off[:, 1] -= off[:, 2] * 0.25 / 32
    out = np.concatenate([pts, off])[:N]
    assert len(out) == N
    out = out[r.permutation(N)]
    if overflow:
      out[N - 1] = [1.0 / 64, 0.25, 4.0, 0.5]
    return out.astype(F)
  P = projections(name)[2]
  x = -2.0 + 92.0 * r.rand(N)
  x = np.where((x >= 0) & (x < 0.25), x + 0.25, x)                    # 128 * bf / x fits uint16 from x = 0.105 on
  pts = np.stack([x, x * (1.6 * r.rand(N) - 0.8), x * (1.0 * r.rand(N) - 0.5), r.rand(N)], axis=1)
  i = 0
  for s in 0.3 + 2.0 * r.rand(300):                                   # several returns along (nearly) one ray
    pts[i + 1, :3] = pts[i + 2, :3] * s if pts[i + 2, 0] * s >= 0.25 else pts[i + 1, :3]
    i += 3
  for _ in range(40):                                                 # behind the camera (q2 < 0), yet inside the image
    pts[i, :3] = point_at(P, 0.2 + 1.1 * r.rand(), 1 + int(r.rand() * (W - 2)), int(r.rand() * H))
    i += 1
  e80 = F(80.0)
  for row in (7, 23, 41, 66):                                         # depth just either side of the 80 m cut, each four times:
    for val, u in ((np.nextafter(e80, F(np.inf)), 20), (e80, 60), (np.nextafter(e80, F(-np.inf)), 100)):      # some are occluded
      pts[i, :3] = point_at(P, float(val), u + row % 5, row)
      i += 1
  pts[i, :3] = point_at(P, 0.0, 37, 11)                               # x = -0.0: kept by x >= 0, depth -0.0, disparity 0
  neg_zero = i
  pts[i + 1, :3] = [np.nan, 1.0, 0.5]
  pts[i + 2, :3] = [12.0, np.nan, 0.5]
  pts[i + 3, :3] = [np.inf, 1.0, 0.5]
  pts[i + 4, :3] = [15.0, np.inf, 0.5]
  order = r.permutation(N)
  out = pts[order].astype(F)
  out[np.nonzero(order == neg_zero)[0][0], 0] = F(-0.0)
  if overflow:
    out[N - 1, :3] = np.array(point_at(P, 0.01, 90, 50), dtype=F)
  return out


def bench_scan(n=125000, seed=7):
  """A seeded scan of the size of a real one for tests/tools/lidar_bench.py, with a KITTI-like calibration at 375 x 1242."""
  r = np.random.RandomState(seed)
  x = -5.0 + 85.0 * r.rand(n)
  pts = np.stack([x, x * (1.8 * r.rand(n) - 0.9), x * (0.3 * r.rand(n) - 0.22), r.rand(n)], axis=1).astype(F)
  axes = np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]])
  c = dict(R=_rot(0.007, -0.004, 0.011).dot(axes), T=np.array([-0.004, -0.076, -0.272]), R_rect_00=_rot(0.002, 0.001, -0.003),
           P_rect_02=np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]]),
           P_rect_03=np.array([[721.5377, 0, 609.5593, -339.5242], [0, 721.5377, 172.854, 2.199936], [0, 0, 1, 0.002729905]]))
  return pts, compose(c), (375, 1242), 721.5377


def checksum(a):
  """(sum, sum of squares) in fp64 over the finite values + the count of the others: a fingerprint of a regenerated array."""
  v = np.asarray(a, dtype=np.float64).ravel()
  ok = np.isfinite(v)
  return np.array([v[ok].sum(), (v[ok] ** 2).sum(), float((~ok).sum())], dtype=np.float64)


# ---- the restatement ------------------------------------------------------------------------------------------------------
def encode(v):
  b = np.ascontiguousarray(v, dtype=F).view(np.uint32)
  return np.where(b & np.uint32(0x80000000), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def decode(k):
  k = np.asarray(k, dtype=np.uint32)
  return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(F)


def project(P, pts, shape):
  """(rows, cols, q2, x) of the points that survive x >= 0 and the bounds, in point order; q in the header's summation order."""
  H, W = shape
  pts = np.asarray(pts, dtype=F)
  keep = pts[:, 0] >= 0                                                # keeps -0.0, drops NaN
  p = pts[keep].astype(np.float64)
  x, y, z = p[:, 0], p[:, 1], p[:, 2]
  with np.errstate(all="ignore"):
    q = [((P[k, 0] * x + P[k, 1] * y) + P[k, 2] * z) + P[k, 3] for k in range(3)]
    a, b = q[0] / q[2], q[1] / q[2]
    u = np.rint(a) - 1.0
    v = np.rint(b) - 1.0
    ok = (u >= 0) & (u < W) & (v >= 0) & (v < H)
  return v[ok].astype(np.int64), u[ok].astype(np.int64), q[2][ok], pts[keep][ok, 0], a[ok], b[ok]


def zbuffer(P, pts, shape, vel_depth):
  """uint32 [H,W]: per pixel the smallest order-preserving key, EMPTY where no point lands."""
  H, W = shape
  rows, cols, q2, x = project(P, pts, shape)[:4]
  with np.errstate(over="ignore"):
    value = x if vel_depth else q2.astype(F)
  z = np.full(H * W, EMPTY, dtype=np.uint32)
  np.minimum.at(z, rows * W + cols, encode(value))
  return z.reshape(H, W)


def depth_from_keys(z):
  d = np.where(z == EMPTY, F(0), decode(z)).astype(F)
  return np.where(d < 0, F(0), d).astype(F)


def depth_map(P, pts, shape, vel_depth):
  """fp32 [H,W]: the nearest return per pixel, 0 where there is none or where it is negative."""
  return depth_from_keys(zbuffer(P, pts, shape, vel_depth))


def disparity(depth, bf64, quantize=True):
  """(depth, disp, disp_u16, overflow count): fp64 division and * 128, truncation; an overflowing pixel is 0 everywhere."""
  depth = np.asarray(depth, dtype=F).copy()
  with np.errstate(all="ignore"):
    d64 = np.float64(bf64) / depth.astype(np.float64)
  d64[(depth == 0) | (depth > F(80))] = 0.0
  over = 128.0 * d64 > 65535
  d64[over] = 0.0
  depth[over] = 0
  q = np.trunc(128.0 * d64).astype(np.uint16)
  disp = (q.astype(F) / F(128)) if quantize else d64.astype(F)
  return depth, disp.astype(F), q, int(over.sum())


def metrics(pred, gt):
  """(fp64 sum of the fp32 |pred - gt| over gt > 0, [count, > 2, > 3, > 4, > 5] as exact integers)."""
  pred, gt = np.asarray(pred, dtype=F), np.asarray(gt, dtype=F)
  m = gt > 0
  e = np.abs((pred[m] - gt[m]).astype(F))
  return float(e.astype(np.float64).sum()), [int(m.sum())] + [int((e > F(t)).sum()) for t in (2, 3, 4, 5)]
