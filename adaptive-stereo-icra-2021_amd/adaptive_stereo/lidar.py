"""Sparse ground-truth depth and disparity from a Velodyne scan, on the device (csrc/lidar.hip).

What the reference's scripts/export_gt_disp.py computes on the host per frame (generate_depth_map :64-117, the conversion to
disparity and to uint16 = 128 * disp :147-162): the scan is projected into the rectified left or right camera, the nearest return
is kept per pixel and depth becomes disparity.  The arithmetic is fixed op by op in include/adaptive_stereo_hip.h; INTEGRATION.md
§E lists where it deliberately differs from the script (duplicates are resolved per pixel; an overflowing pixel is 0 and counted).

  calib = KittiCalibration.from_files("kitti_data_raw/2011_09_26")
  gt = LidarGroundTruth(calib, batch=1)                            # every buffer is allocated here
  points, counts = gt.upload([load_velodyne_bin(path)])            # synchronises (host -> device copies)
  frame = gt.project(points, counts, cam=2, pred_disp=pred)        # no allocation, no synchronisation: graph-capturable
  frame.disp, frame.disp_u16, frame.depth, frame.metrics, frame.overflow

The views a call returns alias the object's buffers: the next call overwrites them.
"""
import os

import numpy as np
import torch

from . import _native as nat
from .collect import gpu_device

_NUMERIC = frozenset("0123456789.e+- ")


def read_calib_file(path):
  """{key: float64 array, or the text when the value is not a list of numbers} of a KITTI calibration file.  A line splits on
  its FIRST colon only (``calib_time: 09-Jan-2012 13:57:47``)."""
  out = {}
  with open(path, "r") as f:
    for line in f:
      if ":" not in line:
        continue
      key, value = line.split(":", 1)
      value = value.strip()
      out[key] = value
      if value and _NUMERIC.issuperset(value):
        try:
          out[key] = np.array([float(t) for t in value.split(" ")], dtype=np.float64)
        except ValueError:
          pass
  return out


class KittiCalibration(object):
  """Velodyne -> image projections of the two rectified colour cameras, float64.  P2, P3: 3x4; image_shape (H, W); fx is the
  left camera's focal length in pixels — the right camera's disparity uses it too, as in the reference."""

  def __init__(self, P2, P3, image_shape, fx, baseline=0.54):
    self.P = {2: np.ascontiguousarray(P2, dtype=np.float64), 3: np.ascontiguousarray(P3, dtype=np.float64)}
    for c, P in self.P.items():
      if P.shape != (3, 4) or not np.isfinite(P).all():
        raise ValueError("KittiCalibration: P%d must be a finite 3x4 matrix (got shape %s)" % (c, P.shape))
    self.image_shape = (int(image_shape[0]), int(image_shape[1]))
    self.fx, self.baseline = float(fx), float(baseline)
    if self.image_shape[0] < 1 or self.image_shape[1] < 1 or not (self.fx > 0 and self.baseline > 0):
      raise ValueError("KittiCalibration: image_shape %r, fx %r and baseline %r must be positive" % (image_shape, fx, baseline))

  @classmethod
  def from_files(cls, calib_dir):
    """From calib_cam_to_cam.txt and calib_velo_to_cam.txt of a KITTI raw date folder."""
    cam = read_calib_file(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
    velo = read_calib_file(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
    velo2cam = np.eye(4)
    velo2cam[:3, :3] = velo["R"].reshape(3, 3)
    velo2cam[:3, 3] = velo["T"]
    rect = np.eye(4)
    rect[:3, :3] = cam["R_rect_00"].reshape(3, 3)
    P = [np.dot(np.dot(cam["P_rect_0%d" % c].reshape(3, 4), rect), velo2cam) for c in (2, 3)]
    shape = cam["S_rect_02"][::-1].astype(np.int32)
    return cls(P[0], P[1], (shape[0], shape[1]), cam["P_rect_02"].reshape(3, 4)[0, 0])

  def velo_to_image(self, cam):
    if cam not in self.P:
      raise ValueError("KittiCalibration: camera %r (2 or 3)" % (cam,))
    return self.P[cam]

  @property
  def bf(self):
    """baseline * fx, one float64 product."""
    return self.baseline * self.fx


def load_velodyne_bin(path):
  """A KITTI .bin scan as a pinned [N,4] fp32 tensor (x forward, y left, z up, reflectance)."""
  a = np.fromfile(path, dtype=np.float32)
  if a.size % 4:
    raise ValueError("load_velodyne_bin: %s holds %d floats, not a multiple of 4" % (path, a.size))
  t = torch.from_numpy(a.reshape(-1, 4))
  return t.pin_memory() if torch.cuda.is_available() else t


class LidarFrame(object):
  """Device views of one project() call.  disp [B,1,h,w] fp32, disp_u16 [B,h,w] uint16 (= 128 * disp, the exported file's
  contents), depth [B,1,h,w] fp32, metrics [B,6] (as_eval_metrics' layout, one row per image) or None, overflow [B] int32."""

  def __init__(self, disp, disp_u16, depth, metrics, overflow):
    self.disp, self.disp_u16, self.depth, self.metrics, self.overflow = disp, disp_u16, depth, metrics, overflow


class LidarGroundTruth(object):
  """Scans [B,N,4] -> sparse ground truth in the image of ``calib``.  project() allocates nothing and never synchronises."""

  def __init__(self, calib, batch=1, max_points=131072, device="cuda"):
    self.calib = calib
    self.H, self.W = calib.image_shape
    self.B, self.max_points = int(batch), int(max_points)
    if self.B < 1 or self.max_points < 1:
      raise ValueError("LidarGroundTruth: batch %d and max_points %d must be positive" % (self.B, self.max_points))
    dev = gpu_device("LidarGroundTruth", device)
    lib = nat.load()
    B, H, W = self.B, self.H, self.W
    ws = lib.as_lidar_resolve_workspace(B, H, W)
    if ws < 0:
      raise ValueError("LidarGroundTruth: a batch of %d frames of %dx%d is outside what the kernels index" % (B, H, W))
    self._zbuf = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    self._depth = torch.empty(B * H * W, dtype=torch.float32, device=dev)
    self._disp = torch.empty(B * H * W, dtype=torch.float32, device=dev)
    self._u16 = torch.empty(B * H * W, dtype=torch.uint16, device=dev)
    self._metrics = torch.zeros(B, 6, dtype=torch.float32, device=dev)
    self._overflow = torch.zeros(B, dtype=torch.int32, device=dev)
    self._ws = torch.empty(ws // 8, dtype=torch.float64, device=dev)
    self._P = {c: torch.from_numpy(calib.velo_to_image(c)).repeat(B, 1, 1).contiguous().to(dev) for c in (2, 3)}
    # staging for upload(): callers with their own device tensors do not need them
    self.points = torch.zeros(B, self.max_points, 4, dtype=torch.float32, device=dev)
    self.counts = torch.zeros(B, dtype=torch.int32, device=dev)
    self.device = self._zbuf.device
    self.clear()

  def clear(self):
    """Empties the z-buffer.  Once at construction: every project() hands it back empty.  Call it after a project() that raised
    from the library."""
    with torch.cuda.device(self.device):
      nat.call("as_lidar_zbuf_clear", nat.ptr(self._zbuf), self.B, self.H, self.W, nat.stream())

  def upload(self, scans):
    """Copies a list of host [N,4] fp32 scans into the staging buffers; returns (points [b,max_points,4], counts [b]) to hand to
    project().  Synchronises.  Rows at or beyond a scan's length keep whatever an earlier scan left there: never read."""
    if not 1 <= len(scans) <= self.B:
      raise RuntimeError("LidarGroundTruth: %d scans, but the buffers were allocated for at most %d" % (len(scans), self.B))
    n = []
    for b, s in enumerate(scans):
      if s.dim() != 2 or s.shape[1] != 4 or s.dtype != torch.float32 or s.shape[0] > self.max_points:
        raise RuntimeError("LidarGroundTruth: scan %d has shape %s and dtype %s, expected fp32 [N <= %d, 4]"
                           % (b, tuple(s.shape), s.dtype, self.max_points))
      self.points[b, :s.shape[0]].copy_(s)
      n.append(s.shape[0])
    self.counts[:len(n)].copy_(torch.tensor(n, dtype=torch.int32))
    return self.points[:len(n)], self.counts[:len(n)]

  def _check(self, points, counts, cam, window, pred_disp):
    if cam not in (2, 3):
      raise ValueError("LidarGroundTruth: camera %r (2 or 3)" % (cam,))
    for name, t, dtype in (("points", points, torch.float32), ("counts", counts, torch.int32), ("pred_disp", pred_disp, torch.float32)):
      if t is None and name == "pred_disp":
        continue
      if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError("adaptive_stereo: %s must live on the GPU (got %s); there is no CPU path"
                           % (name, t.device if torch.is_tensor(t) else type(t).__name__))
      if t.dtype != dtype or not t.is_contiguous() or t.device != self.device:
        raise RuntimeError("LidarGroundTruth: %s must be a contiguous %s tensor on %s (got %s, %s, contiguous=%s)"
                           % (name, dtype, self.device, t.dtype, t.device, t.is_contiguous()))
    if points.dim() != 3 or points.shape[2] != 4 or points.shape[1] < 1:
      raise RuntimeError("LidarGroundTruth: points has shape %s, expected [B,N,4]" % (tuple(points.shape),))
    b, n = points.shape[0], points.shape[1]
    if b < 1 or b > self.B:
      raise RuntimeError("LidarGroundTruth: batch %d, but the buffers were allocated for at most %d" % (b, self.B))
    if n > self.max_points:
      raise RuntimeError("LidarGroundTruth: %d points per scan, but max_points is %d" % (n, self.max_points))
    if tuple(counts.shape) != (b,):
      raise RuntimeError("LidarGroundTruth: counts has shape %s, expected (%d,)" % (tuple(counts.shape), b))
    if points.data_ptr() % 16:
      raise RuntimeError("LidarGroundTruth: points must be 16-byte aligned")
    if window is None:
      window = (0, 0, self.H, self.W)
    i0, j0, h, w = (int(v) for v in window)
    if i0 < 0 or j0 < 0 or h < 1 or w < 1 or i0 + h > self.H or j0 + w > self.W:
      raise RuntimeError("LidarGroundTruth: window %r is not inside the %dx%d image" % (tuple(window), self.H, self.W))
    if pred_disp is not None and tuple(pred_disp.shape) != (b, 1, h, w):
      raise RuntimeError("LidarGroundTruth: pred_disp has shape %s, expected %s" % (tuple(pred_disp.shape), (b, 1, h, w)))
    return b, n, (i0, j0, h, w)

  def project(self, points, counts, cam=2, window=None, vel_depth=True, quantize=True, pred_disp=None):
    """points [B,N,4] fp32 and counts [B] int32 on the device (rows at or beyond counts[b] are never read); window (i0, j0, h, w)
    inside the image, the crop the prediction was made on.  Returns a LidarFrame of views."""
    b, n, (i0, j0, h, w) = self._check(points, counts, cam, window, pred_disp)
    with torch.cuda.device(self.device):                    # the current stream of this object's device, not the caller's
      nat.call("as_lidar_project", nat.ptr(points), nat.ptr(counts), nat.ptr(self._P[cam]), b, n, self.H, self.W,
               1 if vel_depth else 0, nat.ptr(self._zbuf), nat.stream())
      try:
        nat.call("as_lidar_resolve", nat.ptr(self._zbuf), b, self.H, self.W, i0, j0, h, w, self.calib.bf, 1 if quantize else 0,
                 nat.ptr(self._depth), nat.ptr(self._disp), nat.ptr(self._u16), nat.ptr(pred_disp),
                 nat.ptr(self._metrics) if pred_disp is not None else None, nat.ptr(self._ws) if pred_disp is not None else None,
                 nat.ptr(self._overflow), nat.stream())
      except RuntimeError:
        self.clear()                                        # the projection ran and nothing emptied the buffer
        raise
    k = b * h * w
    return LidarFrame(self._disp[:k].view(b, 1, h, w), self._u16[:k].view(b, h, w), self._depth[:k].view(b, 1, h, w),
                      self._metrics[:b] if pred_disp is not None else None, self._overflow[:b])
