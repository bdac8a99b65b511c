"""Host restatement of csrc/pointcloud.hip's contract (include/adaptive_stereo_hip.h, "depth and point cloud from disparity"),
op for op: every fp32 expression below is one numpy float32 operation per written operation, in the written order (numpy never
contracts into an fma), the voxel sums are int64, the voxel means float64.  The GPU tests compare bit for bit against this.

A second, all-float64 version of depth and back-projection (``physics``) says what the numbers mean; the CPU tests hold the
fp32 definition's quantum against it.
"""
import numpy as np

F = np.float32
IDX_LIMIT = F(2 ** 20)
QNAN_BITS = 0x7FC00000


def camera_constants(fx, fy, cx, cy, baseline, s):
  """The fp32 values the kernel receives, each rounded once from the full-resolution (Python float) intrinsics."""
  n = 2 ** s
  return dict(fb=F(fx * baseline), fxs=F(fx / n), fys=F(fy / n), cxs=F(cx / n), cys=F(cy / n))


def _taps(x, s):
  n = 1 << s
  H, W = x.shape[-2:]
  h, w = H >> s, W >> s
  o = n // 2 - 1
  r = (o + n * np.arange(h))[:, None]
  c = (o + n * np.arange(w))[None, :]
  return x[..., r, c], x[..., r, c + 1], x[..., r + 1, c], x[..., r + 1, c + 1]


def downsample(x, s):
  """[..., H, W] float32 -> [..., H >> s, W >> s]: m = ((a + b) + (c + d)) * 0.25f;  s = 0: the pixel itself."""
  x = np.asarray(x)
  assert x.dtype == np.float32
  if s == 0:
    return x.copy()
  a, b, c, d = _taps(x, s)
  with np.errstate(all="ignore"):
    return ((a + b) + (c + d)) * F(0.25)


def points(disp, cam, s, max_depth=100.0, depth_scale=100.0, depth_trunc=80.0):
  """disp [B,1,H,W] float32, cam = camera_constants(...).  Returns a dict of [B,h,w] arrays: depth (clamped, before
  quantisation), q (int64; zeros when depth_scale == 0), x, y, z (float32, computed for every pixel) and valid."""
  assert F(max_depth) * F(depth_scale) <= 65535
  with np.errstate(all="ignore"):
    m = downsample(np.asarray(disp)[:, 0], s)
    d = cam["fb"] / m
    depth = np.minimum(d, F(max_depth))                       # NaN stays NaN
    depth = np.where(depth < 0, F(0), depth).astype(F)
    if depth_scale > 0:
      t = depth * F(depth_scale)
      q = np.where(np.isnan(t), F(0), np.trunc(t)).astype(np.int64)
      z = q.astype(F) / F(depth_scale)
      valid = (q != 0) & ~(z > F(depth_trunc))
    else:
      q = np.zeros(depth.shape, np.int64)
      z = depth
      valid = (z > 0) & (z <= F(depth_trunc))
    h, w = depth.shape[-2:]
    u = np.arange(w, dtype=F)[None, None, :]
    v = np.arange(h, dtype=F)[None, :, None]
    x = ((u - cam["cxs"]) * z) / cam["fxs"]
    y = ((v - cam["cys"]) * z) / cam["fys"]
  x, y = np.broadcast_to(x, z.shape).astype(F), np.broadcast_to(y, z.shape).astype(F)
  return dict(depth=depth, q=q, x=x, y=y, z=z.astype(F), valid=valid)


def organized(p):
  """[B,3,h,w] x, y, z planes with the quiet NaN 0x7FC00000 at invalid pixels."""
  nan = np.array([QNAN_BITS], np.uint32).view(F)[0]
  return np.stack([np.where(p["valid"], p[k], nan) for k in ("x", "y", "z")], axis=1).astype(F)


def colour_bytes(rgb, s):
  """rgb [B,3,H,W] float32 -> [B,3,h,w] int64: (int)(colour * 255.f) clamped to 0..255 (NaN -> 0)."""
  with np.errstate(all="ignore"):
    t = downsample(np.asarray(rgb), s) * F(255)
    return np.where(t >= 255, 255, np.where(t > 0, np.trunc(t), 0)).astype(np.int64)


def voxel_cloud(p, b, voxel_size, colour=None):
  """The voxel filter over image b of points() (colour = colour_bytes(...) or None).  Returns a dict: voxel [n,3] int64 sorted
  by (ix, iy, iz), count [n], xyz [n,3] float32, rgb [n] uint32, n, dropped."""
  valid = p["valid"][b].reshape(-1)
  xyz = np.stack([p[k][b].reshape(-1) for k in ("x", "y", "z")], axis=1)
  with np.errstate(all="ignore"):
    f = np.floor(xyz / F(voxel_size))
    in_range = np.all((f > -IDX_LIMIT) & (f < IDX_LIMIT), axis=1)              # False for NaN
  dropped = int(np.sum(valid & ~in_range))
  keep = valid & in_range
  idx = f[keep].astype(np.int64)
  fixed = np.rint(xyz[keep] * F(65536)).astype(np.int64)                        # llrintf: round half to even
  vox, inv = np.unique(idx, axis=0, return_inverse=True)
  inv = inv.reshape(-1)
  n = vox.shape[0]
  count = np.zeros(n, np.int64)
  S = np.zeros((n, 3), np.int64)
  C = np.zeros((n, 3), np.int64)
  np.add.at(count, inv, 1)
  np.add.at(S, inv, fixed)
  if colour is not None:
    np.add.at(C, inv, colour[b].reshape(3, -1).T[keep])
  mean = (S.astype(np.float64) / (count.astype(np.float64) * 65536.0)[:, None]).astype(F)
  C = C // np.maximum(count, 1)[:, None]
  rgb = ((C[:, 0] << 16) | (C[:, 1] << 8) | C[:, 2]).astype(np.uint32)
  return dict(voxel=vox.reshape(n, 3), count=count, xyz=mean.reshape(n, 3), rgb=rgb, n=n, dropped=dropped)


RECORD = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgb", "<u4")])


def record_bytes(cloud):
  """PointCloud2.data of a voxel_cloud() result (point_step = 16), in the cloud's (sorted) order."""
  rec = np.zeros(cloud["n"], RECORD)
  rec["x"], rec["y"], rec["z"] = cloud["xyz"][:, 0], cloud["xyz"][:, 1], cloud["xyz"][:, 2]
  rec["rgb"] = cloud["rgb"]
  return rec.tobytes()


def sort_cloud(voxel, *others):
  """Rows of a device cloud in the reference's order: sorted by (ix, iy, iz)."""
  voxel = np.asarray(voxel)
  order = np.lexsort((voxel[:, 2], voxel[:, 1], voxel[:, 0]))
  return (voxel[order],) + tuple(np.asarray(o)[order] for o in others)


def physics(disp, fx, fy, cx, cy, baseline, s, max_depth=100.0, depth_scale=100.0):
  """All-float64 depth and back-projection from unrounded intrinsics: depth [B,h,w], q (int64), x, y, z."""
  n = 2 ** s
  d64 = np.asarray(disp)[:, 0].astype(np.float64)
  with np.errstate(all="ignore"):
    if s == 0:
      m = d64
    else:
      a, b, c, d = _taps(d64, s)
      m = (a + b + c + d) / 4.0
    depth = np.minimum(fx * baseline / m, max_depth)
    depth = np.where(depth < 0, 0.0, depth)
    q = np.where(np.isnan(depth), 0.0, np.trunc(depth * depth_scale)).astype(np.int64)
    z = q / depth_scale if depth_scale > 0 else depth
    h, w = depth.shape[-2:]
    u = np.arange(w, dtype=np.float64)[None, None, :]
    v = np.arange(h, dtype=np.float64)[None, :, None]
    x = (u - cx / n) * z / (fx / n)
    y = (v - cy / n) * z / (fy / n)
  return dict(depth=depth, q=q, x=x, y=y, z=z)
