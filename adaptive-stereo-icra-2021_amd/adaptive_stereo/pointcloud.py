"""Metric depth, organised point cloud and voxel-filtered cloud from disparity, on the device (csrc/pointcloud.hip).

What the reference's ROS node computes on the host after the forward pass (ros/stereo_depth_node.py:145-195): bilinear
down-sampling of ``pred_disp_l/0`` to a pyramid level, ``depth = fx * b / disp``, clamp, Open3D's 16-bit depth image,
pinhole back-projection, a voxel filter and ``x, y, z, rgb`` records for a ``PointCloud2`` (ros/open3d_to_ros.py:15-22).
The arithmetic is fixed op by op in include/adaptive_stereo_hip.h; INTEGRATION.md lists the three places where it
deliberately differs from the node.

  cam = StereoCamera.from_dataset(dataset, 375, 1242)
  proj = DepthProjector(375, 1242, cam)                    # every buffer is allocated here
  cloud = proj.voxel_cloud(outputs["pred_disp_l/0"], left) # no allocation, no synchronisation: graph-capturable
  data = cloud.to_pointcloud2_bytes(0)                     # synchronises

With a confidence map (adaptive_stereo.confidence) the cloud keeps only the pixels the network is sure of:

  conf = disparity_confidence(outputs["cost_volume_l/4"], kinds=("mass",))["mass"]
  cloud = proj.voxel_cloud(outputs["pred_disp_l/0"], left, confidence=conf, conf_min=0.8)   # cloud.rejected [B]

The views a method returns alias the projector's buffers: the next call overwrites them.
"""
import ctypes

import torch

from . import _native as nat
from .collect import gpu_device


class StereoCamera(object):
  """Pinhole intrinsics at FULL resolution (pixels) and the stereo baseline in metres."""

  def __init__(self, fx, fy, cx, cy, baseline):
    self.fx, self.fy, self.cx, self.cy, self.baseline = float(fx), float(fy), float(cx), float(cy), float(baseline)
    if not (self.fx > 0 and self.fy > 0 and self.baseline > 0):
      raise ValueError("StereoCamera: fx, fy and baseline must be positive (got %r, %r, %r)" % (fx, fy, baseline))

  @classmethod
  def from_dataset(cls, dataset, height, width):
    """From the intrinsics a StereoDataset records for its data set, scaled to height x width.  A data set without recorded
    intrinsics raises NotImplementedError (StereoDataset.get_intrinsics_normalized)."""
    K = dataset.get_intrinsics(height, width)
    return cls(float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), dataset.get_baseline_meters())

  def native(self, pyramid_scale, max_depth, depth_scale, depth_trunc):
    """as_depth_camera: each constant rounded to fp32 once, here."""
    n = 2 ** pyramid_scale
    return nat.DepthCamera(self.fx * self.baseline, self.fx / n, self.fy / n, self.cx / n, self.cy / n, max_depth, depth_scale,
                           depth_trunc)


class VoxelCloud(object):
  """Device views of one voxel_cloud() call.  records [B,cap,4] int32 (x, y, z as fp32 bits, then R << 16 | G << 8 | B), voxel
  [B,cap,3] int32, count [B,cap] int32, n [B] int32 (rows in use per image), dropped [B] int32, rejected [B] int32 (pixels valid
  by depth that failed the confidence gate; None for a call without one).  Rows at or beyond n[b] hold leftovers of earlier
  calls; the order of rows within an image is unspecified."""

  def __init__(self, batch, records, voxel, count, n, dropped, rejected=None):
    self.batch = batch
    self.records, self.voxel, self.count = records[:batch], voxel[:batch], count[:batch]
    self.n, self.dropped = n[:batch], dropped[:batch]
    self.rejected = None if rejected is None else rejected[:batch]

  @property
  def xyz(self):
    return self.records.view(torch.float32)[..., :3]

  def trim(self):
    """Synchronises.  Per image a dict of tensors cut to n[b]: records, xyz, rgb, voxel, count, and dropped as an int."""
    n, dropped = self.n.tolist(), self.dropped.tolist()
    out = []
    for b in range(self.batch):
      k = min(n[b], self.records.shape[1])
      out.append(dict(records=self.records[b, :k], xyz=self.xyz[b, :k], rgb=self.records[b, :k, 3], voxel=self.voxel[b, :k],
                      count=self.count[b, :k], dropped=dropped[b]))
    return out

  def to_pointcloud2_bytes(self, b):
    """Synchronises.  The n[b] * 16 bytes of sensor_msgs/PointCloud2.data for image b (point_step = 16, fields x, y, z float32
    at offsets 0, 4, 8 and rgb uint32 at 12, little endian)."""
    k = min(int(self.n[b]), self.records.shape[1])
    return self.records[b, :k].cpu().numpy().tobytes()


class DepthProjector(object):
  """Disparity [B,1,H,W] -> depth / organised cloud / voxel cloud at pyramid level ``pyramid_scale`` (0, 1 or 2).  The defaults
  are the node's Config.  depth(), organized() and voxel_cloud() allocate nothing and never synchronise.

  organized() and voxel_cloud() take a confidence map [B,hc,wc] or [B,1,hc,wc] of any coarse size together with conf_min: the
  map is up-sampled to (h, w) into ``confidence_level`` (as_upsample_bilinear_fwd, gain 1) and a pixel that is valid by depth is
  kept only when its confidence there is >= conf_min (a NaN confidence rejects it)."""

  def __init__(self, height, width, camera, batch=1, pyramid_scale=2, max_depth=100.0, depth_scale=100.0, depth_trunc=80.0,
               voxel_size=0.15, device="cuda", table_slots=None):
    if pyramid_scale not in (0, 1, 2):
      raise ValueError("DepthProjector: pyramid_scale %r (0, 1 or 2)" % (pyramid_scale,))
    if not (max_depth > 0 and depth_scale >= 0 and depth_trunc > 0 and voxel_size > 0):
      raise ValueError("DepthProjector: max_depth, depth_trunc and voxel_size must be positive, depth_scale >= 0")
    if max_depth * depth_scale > 65535:
      raise ValueError("DepthProjector: max_depth %g * depth_scale %g = %g does not fit a 16-bit depth image (<= 65535)"
                       % (max_depth, depth_scale, max_depth * depth_scale))
    self.H, self.W, self.B, self.s = int(height), int(width), int(batch), int(pyramid_scale)
    self.h, self.w = self.H >> self.s, self.W >> self.s
    if self.B < 1 or self.h < 1 or self.w < 1:
      raise ValueError("DepthProjector: batch %d of %dx%d at scale %d has no output pixels" % (self.B, self.H, self.W, self.s))
    lib = nat.load()
    points = self.h * self.w
    if table_slots is None:
      table_slots = lib.as_voxel_table_slots(points)
    table_slots = int(table_slots)
    if table_slots < 64 or table_slots & (table_slots - 1) or table_slots < points:
      raise ValueError("DepthProjector: table_slots %d must be a power of two >= max(64, h*w = %d)" % (table_slots, points))
    self.slots, self.cap = table_slots, points
    self.voxel_size = float(voxel_size)
    self.camera = camera
    self._cam = camera.native(self.s, max_depth, depth_scale, depth_trunc)
    self.device = dev = gpu_device("DepthProjector", device)
    B, h, w = self.B, self.h, self.w
    self._depth = torch.empty(B, 1, h, w, dtype=torch.float32, device=dev)
    self._xyz = torch.empty(B, 3, h, w, dtype=torch.float32, device=dev)
    self._table = torch.empty(lib.as_voxel_table_bytes(B, self.slots), dtype=torch.uint8, device=dev)
    self._records = torch.zeros(B, self.cap, 4, dtype=torch.int32, device=dev)
    self._voxel = torch.zeros(B, self.cap, 3, dtype=torch.int32, device=dev)
    self._count = torch.zeros(B, self.cap, dtype=torch.int32, device=dev)
    self._n = torch.zeros(B, dtype=torch.int32, device=dev)
    self._dropped = torch.zeros(B, dtype=torch.int32, device=dev)
    self._conf = torch.zeros(B, 1, h, w, dtype=torch.float32, device=dev)
    self._rejected = torch.zeros(B, dtype=torch.int32, device=dev)
    self._conf_batch = 0
    with torch.cuda.device(dev):
      # once: as_voxel_cloud_finalize hands back empty every slot it read, so no later call clears the table
      nat.call("as_voxel_table_clear", nat.ptr(self._table), B, self.slots, nat.stream())

  def _check(self, disp, left_img):
    nat.require_gpu(disp, left_img)
    if disp.dim() != 4 or tuple(disp.shape[1:]) != (1, self.H, self.W):
      raise RuntimeError("DepthProjector: disp has shape %s, expected [B,1,%d,%d]" % (tuple(disp.shape), self.H, self.W))
    b = disp.shape[0]
    if b < 1 or b > self.B:
      raise RuntimeError("DepthProjector: batch %d, but the buffers were allocated for at most %d" % (b, self.B))
    if left_img is not None and tuple(left_img.shape) != (b, 3, self.H, self.W):
      raise RuntimeError("DepthProjector: left_img has shape %s, expected %s" % (tuple(left_img.shape), (b, 3, self.H, self.W)))
    for t in (disp, left_img):
      if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != self._depth.device):
        raise RuntimeError("DepthProjector: inputs must be contiguous fp32 tensors on %s (got %s, %s, contiguous=%s)"
                           % (self._depth.device, t.dtype, t.device, t.is_contiguous()))
    return b

  @property
  def confidence_level(self):
    """[B,1,h,w]: the confidence the last gated call compared with conf_min, at the pyramid level's resolution."""
    return self._conf[:self._conf_batch]

  def _check_confidence(self, b, confidence, conf_min):
    """The coarse size (hc, wc) of a usable confidence map; None for a call without a gate."""
    if confidence is None and conf_min is None:
      return None
    if confidence is None or conf_min is None:
      raise ValueError("DepthProjector: confidence and conf_min go together (got confidence %s, conf_min %r)"
                       % ("None" if confidence is None else tuple(confidence.shape), conf_min))
    nat.require_gpu(confidence)
    shape = tuple(confidence.shape)
    if confidence.dim() == 4 and shape[1] == 1:
      shape = (shape[0],) + shape[2:]
    if len(shape) != 3 or shape[0] != b or shape[1] < 1 or shape[2] < 1:
      raise RuntimeError("DepthProjector: confidence has shape %s, expected [%d,hc,wc] or [%d,1,hc,wc]"
                         % (tuple(confidence.shape), b, b))
    if confidence.dtype != torch.float32 or not confidence.is_contiguous() or confidence.device != self._depth.device:
      raise RuntimeError("DepthProjector: confidence must be a contiguous fp32 tensor on %s (got %s, %s, contiguous=%s)"
                         % (self._depth.device, confidence.dtype, confidence.device, confidence.is_contiguous()))
    if conf_min != conf_min:
      raise ValueError("DepthProjector: conf_min is NaN")
    return shape[1:]

  def _run(self, disp, left_img, depth, xyz, table, confidence=None, conf_min=None):
    b = self._check(disp, left_img)
    coarse = self._check_confidence(b, confidence, conf_min)
    outs = (nat.ptr(self._depth) if depth else None, nat.ptr(self._xyz) if xyz else None, self.voxel_size,
            nat.ptr(self._table) if table else None, self.slots)
    with torch.cuda.device(self.device):                    # the current stream of the projector's device, not the caller's
      if coarse is None:
        nat.call("as_disp_to_points", nat.ptr(disp), nat.ptr(left_img), b, self.H, self.W, self.s, ctypes.byref(self._cam),
                 *(outs + (nat.stream(),)))
      else:
        nat.call("as_upsample_bilinear_fwd", nat.ptr(confidence), b, coarse[0], coarse[1], nat.ptr(self._conf), self.h, self.w, 1.0,
                 nat.stream())
        self._conf_batch = b
        nat.call("as_disp_to_points_gated", nat.ptr(disp), nat.ptr(left_img), nat.ptr(self._conf), float(conf_min), b, self.H,
                 self.W, self.s, ctypes.byref(self._cam), *(outs + (nat.ptr(self._rejected), nat.stream())))
    return b

  def depth(self, disp):
    """Clamped metric depth [B,1,h,w] (before quantisation; NaN where the disparity is NaN)."""
    b = self._run(disp, None, True, False, False)
    return self._depth[:b]

  def organized(self, disp, confidence=None, conf_min=None):
    """(xyz [B,3,h,w] with NaN at invalid pixels, depth [B,1,h,w]).  With confidence and conf_min the pixels below the gate are
    NaN in xyz too (their depth is written as ever); ``rejected`` [B] counts them."""
    b = self._run(disp, None, True, True, False, confidence, conf_min)
    return self._xyz[:b], self._depth[:b]

  @property
  def rejected(self):
    """[B] int32: per image the pixels the last gated call found valid by depth and below conf_min."""
    return self._rejected[:self._conf_batch]

  def voxel_cloud(self, disp, left_img=None, confidence=None, conf_min=None):
    """The voxel-filtered cloud of each image, coloured by left_img [B,3,H,W] in [0,1] when given; with confidence and conf_min,
    of the pixels at or above the gate (VoxelCloud.rejected counts the others)."""
    b = self._run(disp, left_img, False, False, True, confidence, conf_min)
    with torch.cuda.device(self.device):
      try:
        nat.call("as_voxel_cloud_finalize", nat.ptr(self._table), b, self.slots, self.cap, nat.ptr(self._records),
                 nat.ptr(self._voxel), nat.ptr(self._count), nat.ptr(self._n), nat.ptr(self._dropped), nat.stream())
      except RuntimeError:
        # the insert ran and nothing emptied the table: clear it, or the next frame would see this one's voxels
        nat.call("as_voxel_table_clear", nat.ptr(self._table), self.B, self.slots, nat.stream())
        raise
    return VoxelCloud(b, self._records, self._voxel, self._count, self._n, self._dropped,
                      None if confidence is None else self._rejected)
