"""Stereo rectification of raw camera pairs on the device (csrc/rectify.hip): the stage between "the camera delivers bytes" and
the network's input.  Everything else here assumes rectified images; a rig of one's own, or KITTI raw *extract* drives (1392x512,
unrectified, with calib_cam_to_cam.txt), are not.

  calib = KittiRawRectification.from_file("2011_09_26/calib_cam_to_cam.txt")          # cameras 2 and 3
  rect = Rectifier(calib.view_l, calib.view_r, calib.raw_size, batch=B)                # every buffer is allocated here
  left, right = rect(raw_l, raw_r)                      # uint8 [B,H0,W0,3] -> fp32 [B,3,H,W]; enqueue only, capturable
  proj = DepthProjector(H, W, rect.camera, batch=B)     # pointcloud: the intrinsics and the baseline of the produced window

  R1, R2, P1, P2 = stereo_rectify(cam_l, cam_r, R, T)   # a rig of one's own: RawCamera x 2 and the pose of the right camera
  rect = Rectifier(RectifiedView(cam_l, R1, P1), RectifiedView(cam_r, R2, P2), cam_l.size)

  both = BothViewInference(feature_net, stereo_net, H, W, batch=B)
  chain = RectifiedInference(both, rect).capture()      # raw bytes in, both's tuple out: one hipGraph replay
  disp_l, disp_r, chk, filled_l = chain(raw_l, raw_r)

The calibration never changes, so the gather belongs in the captured graph; the kernel recomputes the coordinates per frame (3 B
read, 12 B written per pixel; a stored map would add 8 B).  The arithmetic is fixed op by op in include/adaptive_stereo_hip.h.
All host geometry is fp64 numpy; a view's matrix is inverted in fp64 and rounded to fp32 once.  Sizes are (height, width).

Not handled: fisheye models, vertical rigs, and the fold-back of a strongly negative radial term far outside the field of view
(the forward polynomial is evaluated wherever a ray points, as OpenCV does: such a pixel counts as valid).  There is no CPU path.
"""
import numpy as np
import torch

from . import _native as nat
from . import lidar
from .capture import refuse_nested, warm_up_and_capture
from .collect import check_f32, check_shape, check_u8, gpu_device
from .pointcloud import StereoCamera


def _matrix(who, name, a, shape):
  a = np.array(a, dtype=np.float64)
  if a.shape != shape or not np.isfinite(a).all():
    raise ValueError("%s: %s must be a finite %s matrix (got shape %s)" % (who, name, "x".join(str(s) for s in shape), a.shape))
  return a


def _size(who, name, size):
  try:
    h, w = int(size[0]), int(size[1])
    ok = len(size) == 2 and h == size[0] and w == size[1] and h >= 1 and w >= 1
  except (TypeError, ValueError, IndexError):
    ok = False
  if not ok:
    raise ValueError("%s: %s must be (height, width), both at least 1 (got %r)" % (who, name, size))
  return h, w


class RawCamera(object):
  """A camera as calibrated: K 3x3, D the distortion coefficients in OpenCV's order (k1, k2, p1, p2[, k3[, k4, k5, k6]]: 4, 5 or
  8 of them), size (height, width) of its images."""

  def __init__(self, K, D, size):
    self.K = _matrix("RawCamera", "K", K, (3, 3))
    if not (self.K[0, 0] > 0 and self.K[1, 1] > 0) or self.K[0, 1] != 0 or (self.K[1, 0], self.K[2, 0], self.K[2, 1], self.K[2, 2]) != (0, 0, 0, 1):
      raise ValueError("RawCamera: K must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] with positive focal lengths (got %r)" % (self.K.tolist(),))
    D = np.array(D, dtype=np.float64).reshape(-1)
    if D.size not in (4, 5, 8) or not np.isfinite(D).all():
      raise ValueError("RawCamera: D must hold 4, 5 or 8 finite coefficients (got %d)" % D.size)
    self.D = np.zeros(8, dtype=np.float64)                     # absent coefficients are 0
    self.D[:D.size] = D
    self.size = _size("RawCamera", "size", size)

  def project(self, xyz):
    """The forward model in fp64: points [...,3] in this camera's frame -> raw pixels [...,2].  No iteration anywhere."""
    xyz = np.asarray(xyz, dtype=np.float64)
    k1, k2, p1, p2, k3, k4, k5, k6 = self.D
    xn, yn = xyz[..., 0] / xyz[..., 2], xyz[..., 1] / xyz[..., 2]
    r2 = xn * xn + yn * yn
    rad = (((k3 * r2 + k2) * r2 + k1) * r2 + 1.0) / (((k6 * r2 + k5) * r2 + k4) * r2 + 1.0)
    xd = xn * rad + 2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn)
    yd = yn * rad + p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn
    return np.stack([self.K[0, 0] * xd + self.K[0, 2], self.K[1, 1] * yd + self.K[1, 2]], axis=-1)


class RectifiedView(object):
  """A raw camera, the rotation R_rect that takes its frame to the rectified one, and the rectified projection P_rect (3x4:
  [[f, 0, cx, f*tx], [0, f, cy, 0], [0, 0, 1, 0]]).  size: (height, width) of the full rectified image, the raw size when None."""

  def __init__(self, raw, R_rect, P_rect, size=None):
    if not isinstance(raw, RawCamera):
      raise ValueError("RectifiedView: raw must be a RawCamera (got %s)" % type(raw).__name__)
    self.raw = raw
    self.R = _matrix("RectifiedView", "R_rect", R_rect, (3, 3))
    if np.abs(self.R.dot(self.R.T) - np.eye(3)).max() > 1e-6 or np.linalg.det(self.R) < 0:
      raise ValueError("RectifiedView: R_rect is not a rotation")
    self.P = _matrix("RectifiedView", "P_rect", P_rect, (3, 4))
    if not (self.P[0, 0] > 0 and self.P[1, 1] > 0) or tuple(self.P[2]) != (0, 0, 1, 0) or self.P[0, 1] != 0 or self.P[1, 0] != 0:
      raise ValueError("RectifiedView: P_rect must be [[fx, 0, cx, fx*tx], [0, fy, cy, ty], [0, 0, 1, 0]] (got %r)" % (self.P.tolist(),))
    self.size = raw.size if size is None else _size("RectifiedView", "size", size)

  def inverse(self):
    """fp64 inv(P_rect[:3,:3] . R_rect): a rectified pixel (u, v, 1) -> a ray in the raw camera's frame."""
    return np.linalg.inv(self.P[:, :3].dot(self.R))

  def native(self):
    """as_rectify_camera: every constant rounded to fp32 once, here."""
    cam = nat.RectifyCamera()
    cam.m[:] = [float(v) for v in self.inverse().astype(np.float32).reshape(-1)]
    K, D = self.raw.K, self.raw.D
    cam.fx, cam.fy, cam.cx, cam.cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    cam.k1, cam.k2, cam.p1, cam.p2, cam.k3, cam.k4, cam.k5, cam.k6 = [float(v) for v in D]
    return cam

  def project(self, xyz):
    """fp64: points [...,3] in THIS raw camera's frame -> rectified pixels [...,2]: P_rect[:, :3] . R_rect . x.  P_rect[:, 3] is
    where this camera stands in the rig's reference frame (f * tx); a point given in the camera's own frame already has it."""
    p = np.asarray(xyz, dtype=np.float64).dot(self.R.T).dot(self.P[:, :3].T)
    return p[..., :2] / p[..., 2:]


def rodrigues(v):
  """Rotation vector -> matrix, or matrix -> vector (angle below pi), fp64."""
  v = np.asarray(v, dtype=np.float64)
  if v.shape == (3, 3):
    c = min(1.0, max(-1.0, (np.trace(v) - 1.0) / 2.0))
    axis = np.array([v[2, 1] - v[1, 2], v[0, 2] - v[2, 0], v[1, 0] - v[0, 1]]) / 2.0
    s = np.linalg.norm(axis)
    theta = np.arctan2(s, c)
    return axis * (theta / s) if s > 1e-300 else np.zeros(3)
  theta = np.linalg.norm(v)
  if theta < 1e-300:
    return np.eye(3)
  k = v / theta
  Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
  return np.eye(3) + np.sin(theta) * Kx + (1.0 - np.cos(theta)) * Kx.dot(Kx)


def stereo_rectify(cam_l, cam_r, R, T, new_size=None):
  """(R1, R2, P1, P2) of a horizontal rig, fp64.  R, T: the pose of the left camera's frame in the right one, x_r = R x_l + T
  (OpenCV's stereoCalibrate), so T[0] < 0 for a right camera to the right.

  Rotations (Bouguet): each camera turns by half of R, towards the other, which makes the image planes parallel with the
  least turn of either; then both turn by the smallest rotation that lays the baseline on the x axis.
  One focal length f for both views: the smaller of the two fy, which samples neither raw image finer than it was taken.
  One principal point for both views, so that a point at infinity has disparity 0 and equal rows: the ray through the centre of
  each RAW image ((W0-1)/2, (H0-1)/2, distortion left aside) is rotated into the rectified frame, and (cx, cy) is chosen so that
  the mean of the two lands on the centre of the new image ((W-1)/2, (H-1)/2); new_size (height, width) is the left raw size when
  None.  P1 = [f 0 cx 0; 0 f cy 0; 0 0 1 0]; P2 the same with P2[0,3] = -f * |T|."""
  for name, c in (("cam_l", cam_l), ("cam_r", cam_r)):
    if not isinstance(c, RawCamera):
      raise ValueError("stereo_rectify: %s must be a RawCamera (got %s)" % (name, type(c).__name__))
  R = _matrix("stereo_rectify", "R", R, (3, 3))
  T = _matrix("stereo_rectify", "T", np.asarray(T, dtype=np.float64).reshape(-1), (3,))
  if np.abs(R.dot(R.T) - np.eye(3)).max() > 1e-6 or np.linalg.det(R) < 0:
    raise ValueError("stereo_rectify: R is not a rotation")
  r_r = rodrigues(-0.5 * rodrigues(R))                       # R^(-1/2): what the right camera turns by; the left by its transpose
  t = r_r.dot(T)
  norm = np.linalg.norm(t)
  if not (norm > 0 and t[0] < 0 and abs(t[0]) >= max(abs(t[1]), abs(t[2]))):
    raise ValueError("stereo_rectify: T %r is not the baseline of a horizontal rig with the first camera on the left (after the half "
                     "turn it is %r; vertical rigs are not handled)" % (T.tolist(), t.tolist()))
  w = np.cross(t, np.array([-1.0, 0.0, 0.0]))                # turns t onto -x
  nw = np.linalg.norm(w)
  if nw > 0:
    w = w * (np.arccos(min(1.0, abs(t[0]) / norm)) / nw)
  wR = rodrigues(w)
  R1, R2 = wR.dot(r_r.T), wR.dot(r_r)
  f = min(cam_l.K[1, 1], cam_r.K[1, 1])
  H, W = cam_l.size if new_size is None else _size("stereo_rectify", "new_size", new_size)
  c = np.zeros(2)
  for cam, Rc in ((cam_l, R1), (cam_r, R2)):
    ray = Rc.dot(np.linalg.inv(cam.K).dot(np.array([(cam.size[1] - 1) / 2.0, (cam.size[0] - 1) / 2.0, 1.0])))
    c += 0.5 * (np.array([(W - 1) / 2.0, (H - 1) / 2.0]) - f * ray[:2] / ray[2])
  P1 = np.array([[f, 0.0, c[0], 0.0], [0.0, f, c[1], 0.0], [0.0, 0.0, 1.0, 0.0]])
  P2 = P1.copy()
  P2[0, 3] = -f * norm
  return R1, R2, P1, P2


def stereo_camera(view_l, view_r, window=None):
  """The pointcloud.StereoCamera of a window (i0, j0, H, W) of a rectified pair: fx, fy from P, cx - j0, cy - i0, and the
  baseline from the two P[0,3] / P[0,0].  ValueError when the two views do not share fx, fy, cx and cy."""
  Pl, Pr = view_l.P, view_r.P
  if (Pl[0, 0], Pl[1, 1], Pl[0, 2], Pl[1, 2]) != (Pr[0, 0], Pr[1, 1], Pr[0, 2], Pr[1, 2]):
    raise ValueError("adaptive_stereo.rectify: the two views must share fx, fy, cx and cy (left %r, right %r): with different ones a "
                     "point at infinity has a disparity, or the rows differ"
                     % ((Pl[0, 0], Pl[1, 1], Pl[0, 2], Pl[1, 2]), (Pr[0, 0], Pr[1, 1], Pr[0, 2], Pr[1, 2])))
  baseline = Pl[0, 3] / Pl[0, 0] - Pr[0, 3] / Pr[0, 0]
  if not baseline > 0:
    raise ValueError("adaptive_stereo.rectify: the baseline from the two P[0,3] / P[0,0] is %r; view_r must be the camera on the "
                     "right" % (baseline,))
  i0, j0 = (0, 0) if window is None else (window[0], window[1])
  return StereoCamera(Pl[0, 0], Pl[1, 1], Pl[0, 2] - j0, Pl[1, 2] - i0, baseline)


class KittiRawRectification(object):
  """The two views of a KITTI raw calibration file (calib_cam_to_cam.txt): view_l, view_r (RectifiedView), raw_size and
  rect_size (height, width), camera (the pointcloud.StereoCamera of the full rectified image)."""

  def __init__(self, view_l, view_r):
    self.view_l, self.view_r = view_l, view_r
    self.raw_size, self.rect_size = view_l.raw.size, view_l.size
    self.camera = stereo_camera(view_l, view_r)

  @classmethod
  def from_file(cls, path, cams=(2, 3)):
    """Reads K_0c, D_0c, S_0c, R_rect_0c, P_rect_0c and S_rect_0c of the two cameras (left, right).  S is width, height."""
    calib = lidar.read_calib_file(path)
    views = []
    for c in cams:
      vals = {}
      for key, n in (("K", 9), ("D", 5), ("S", 2), ("R_rect", 9), ("P_rect", 12), ("S_rect", 2)):
        name = "%s_0%d" % (key, c)
        v = calib.get(name)
        if not isinstance(v, np.ndarray) or v.size != n:
          raise ValueError("KittiRawRectification: %s has no entry %s of %d numbers" % (path, name, n))
        vals[key] = v
      raw = RawCamera(vals["K"].reshape(3, 3), vals["D"], (vals["S"][1], vals["S"][0]))
      views.append(RectifiedView(raw, vals["R_rect"].reshape(3, 3), vals["P_rect"].reshape(3, 4), (vals["S_rect"][1], vals["S_rect"][0])))
    if views[0].raw.size != views[1].raw.size or views[0].size != views[1].size:
      raise ValueError("KittiRawRectification: cameras %r differ in size" % (tuple(cams),))
    return cls(views[0], views[1])


class Rectifier(object):
  """Raw uint8 pairs [batch,H0,W0,channels] -> rectified fp32 pairs [batch,3,H,W] in [0, 1], one launch for both cameras and the
  batch.  raw_size: (H0, W0); window: (i0, j0, H, W) of the rectified image, any window, the views' full size at (0, 0) when None.
  Every buffer is allocated here; as_rectify_map runs once per camera here, which gives valid_l, valid_r (fp32 1.0 / 0.0
  [batch,1,H,W]: where the window sees the raw image; they depend on the calibration and the window only), maps() and
  valid_fraction().  A pixel that is not valid carries `fill` in every plane.  ``camera`` is the pointcloud.StereoCamera of the
  produced window."""

  def __init__(self, view_l, view_r, raw_size, window=None, batch=1, channels=3, fill=0.0, device="cuda"):
    for name, v in (("view_l", view_l), ("view_r", view_r)):
      if not isinstance(v, RectifiedView):
        raise ValueError("Rectifier: %s must be a RectifiedView (got %s)" % (name, type(v).__name__))
    self.view_l, self.view_r = view_l, view_r
    self.H0, self.W0 = _size("Rectifier", "raw_size", raw_size)
    stereo_camera(view_l, view_r)                              # (raises when the views do not belong together)
    if window is None:
      window = (0, 0) + tuple(view_l.size)
    try:
      i0, j0, H, W = [int(v) for v in window]
      ok = all(int(v) == v for v in window) and H >= 1 and W >= 1 and abs(i0) <= 2 ** 30 and abs(j0) <= 2 ** 30 and H * W < 2 ** 30
    except (TypeError, ValueError):
      ok = False
    if not ok:
      raise ValueError("Rectifier: window must be integers (i0, j0, H, W) with H, W >= 1 (got %r)" % (window,))
    self.i0, self.j0, self.H, self.W = i0, j0, H, W
    self.B, self.C, self.fill = int(batch), int(channels), float(fill)
    if self.B < 1 or 2 * self.B > 65535 or self.C not in (1, 3):
      raise ValueError("Rectifier: batch %r (1 .. 32767), channels %r (1 or 3)" % (batch, channels))
    self.device = dev = gpu_device("Rectifier", device)
    self.camera = stereo_camera(view_l, view_r, (i0, j0, H, W))
    self._cams = (view_l.native(), view_r.native())
    self._out = torch.zeros(2, self.B, 3, H, W, dtype=torch.float32, device=dev)
    self._maps = torch.zeros(2, 2, H, W, dtype=torch.float32, device=dev)          # [camera][x, y]
    valid = torch.zeros(2, 1, 1, H, W, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
      for c in range(2):
        nat.call("as_rectify_map", self._cams[c], self.H0, self.W0, i0, j0, H, W, nat.ptr(self._maps[c, 0]), nat.ptr(self._maps[c, 1]),
                 nat.ptr(valid[c]), nat.stream())
    self._valid = valid.expand(2, self.B, 1, H, W).contiguous()
    self.valid_l, self.valid_r = self._valid[0], self._valid[1]

  def maps(self):
    """((map_x_l, map_y_l), (map_x_r, map_y_r)): fp32 [H,W], the raw pixel each output pixel samples, exactly as the frame kernel
    computes it (NaN and infinities included where the window reaches a rotated camera's horizon)."""
    return (self._maps[0, 0], self._maps[0, 1]), (self._maps[1, 0], self._maps[1, 1])

  def valid_fraction(self):
    """Synchronises.  (left, right): the share of the window's pixels that see the raw image."""
    n = (self._valid[:, 0] > 0).sum(dim=(1, 2, 3)).cpu()      # counted: exact
    return int(n[0]) / float(self.H * self.W), int(n[1]) / float(self.H * self.W)

  def _check_raw(self, name, t):
    shape = (self.B, self.H0, self.W0, self.C)
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
      raise RuntimeError("adaptive_stereo: tensors must live on the GPU (got %s for %s); there is no CPU path"
                         % (getattr(t, "device", type(t)), name))
    check_u8("Rectifier", name, t, shape, self._out.device)

  def __call__(self, raw_l, raw_r, out=None):
    """-> (left, right) fp32 [B,3,H,W]: this object's buffers, or `out` = (left, right), e.g. BothViewInference.inputs()."""
    self._check_raw("raw_l", raw_l)
    self._check_raw("raw_r", raw_r)
    if out is None:
      left, right = self._out[0], self._out[1]
    else:
      left, right = out
      for name, t in (("out[0]", left), ("out[1]", right)):
        check_f32("Rectifier", name, t, ((4,), "[B,3,H,W]"), device=self._out.device)
        check_shape("Rectifier", name, t, (self.B, 3, self.H, self.W), self._out.device)
    with torch.cuda.device(self.device):
      nat.call("as_rectify_pair", nat.ptr(raw_l), nat.ptr(raw_r), self.B, self.H0, self.W0, self.C, self._cams[0], self._cams[1],
               self.i0, self.j0, self.H, self.W, self.fill, nat.ptr(left), nat.ptr(right), nat.stream())
    return left, right


class RectifiedInference(object):
  """Raw bytes in, `inner`'s result out: the raw uint8 frames are copied into static buffers, rectified straight into
  ``inner.inputs()`` and `inner`'s chain runs on them.  inner: a consistency.BothViewInference or a
  disp_filter.FilteredBothViewInference, not captured itself; the result is its tuple, views of its buffers that the next call
  overwrites.  After capture() a call is two copies of raw bytes and one graph replay (one stream, no forks).  The raw tensors
  may be overwritten as soon as the call returns.

  Where ``rectifier.valid_l`` has zeros (a window that leaves the raw image) those pixels carry `fill`, the network sees a flat
  border there and predicts something for it: gate them as any other confidence, ``proj.voxel_cloud(disp_l, left,
  confidence=rectifier.valid_l, conf_min=1.0)`` (pointcloud.DepthProjector), or multiply valid_l into the LRCheck's valid_l."""

  def __init__(self, inner, rectifier):
    if not isinstance(rectifier, Rectifier):
      raise ValueError("RectifiedInference: rectifier must be a Rectifier (got %s)" % type(rectifier).__name__)
    if not (hasattr(inner, "inputs") and hasattr(inner, "run_static")):
      raise ValueError("RectifiedInference: inner must be a BothViewInference or a FilteredBothViewInference (got %s)" % type(inner).__name__)
    left, right = inner.inputs()
    shape = (rectifier.B, 3, rectifier.H, rectifier.W)
    if tuple(left.shape) != shape or left.device != rectifier._out.device:
      raise ValueError("RectifiedInference: the rectifier produces %s on %s, inner takes %s on %s"
                       % (shape, rectifier._out.device, tuple(left.shape), left.device))
    self.inner, self.rectifier = inner, rectifier
    r = rectifier
    self._raw = torch.zeros(2, r.B, r.H0, r.W0, r.C, dtype=torch.uint8, device=left.device)
    self._graph = None
    self._graph_result = None
    self._capture_origin = None

  def _eager(self):
    self.rectifier(self._raw[0], self._raw[1], out=self.inner.inputs())
    return self.inner.run_static()

  @torch.no_grad()
  def __call__(self, raw_l, raw_r):
    self.rectifier._check_raw("raw_l", raw_l)
    self.rectifier._check_raw("raw_r", raw_r)
    self._raw[0].copy_(raw_l)
    self._raw[1].copy_(raw_r)
    if self._graph is not None:
      self._graph.replay()
      return self._graph_result
    return self._eager()

  @torch.no_grad()
  def capture(self, raw_l=None, raw_r=None, warmup=2):
    """Records rectification and inner's chain once into a hipGraph; raw_l, raw_r: a pair to warm up on (zeros otherwise)."""
    refuse_nested("RectifiedInference.capture")
    if raw_l is not None:
      self.rectifier._check_raw("raw_l", raw_l)
      self.rectifier._check_raw("raw_r", raw_r)
      self._raw[0].copy_(raw_l)
      self._raw[1].copy_(raw_r)
    # (warm-up: the first call records inner's plan, the second runs it)
    self._graph, self._graph_result = warm_up_and_capture(self._eager, max(2, warmup), self._eager, owner=self)
    return self
