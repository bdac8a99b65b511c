"""Times the depth / point-cloud stage (csrc/pointcloud.hip) at 375x1242 with HIP events: as_disp_to_points + as_voxel_cloud_finalize
with and without colour, for B in {1, 4} and pyramid scale in {2, 0}, on a near-plane frame (a few hundred crowded voxels: atomics
of many lanes on one address) and on a random frame (every point a voxel of its own: scattered atomics).  Beside them, in the same
run: an eager-PyTorch restatement of the pipeline on the GPU (interpolate, divide, floor, unique + index_add_; it lives here, not
in the product), the host path the reference's node takes (.cpu() + numpy, tests/pointcloud_ref.py) and the forward-only time per
pair of train.process_batch for scale.  20 warm-up and 100 timed calls, five repeats: median and [min .. max] of the repeats
(the host path: wall clock over five single calls).  There is no pass/fail time.

usage (GPU box): python tests/tools/time_pointcloud.py [--out profiles/pointcloud_timing.txt]
"""
import argparse
import ctypes
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "adaptive-stereo-icra-2021_amd"))
sys.path.insert(0, os.path.join(HERE, ".."))
import numpy as np
import torch
import torch.nn.functional as F

from adaptive_stereo import _native as nat
from adaptive_stereo.pointcloud import DepthProjector, StereoCamera
import pointcloud_ref as pr

DEV = "cuda:0"
H, W = 375, 1242
WARM, CALLS, REPEATS = 20, 100, 5
CAM = StereoCamera(0.5885 * W, 1.9501 * H, 0.4972 * W, 0.4972 * H, 0.54)        # the KITTI intrinsics StereoDataset records
VOXEL, MAX_DEPTH, SCALE, TRUNC = 0.15, 100.0, 100.0, 80.0                       # the node's Config


def frame(kind, B, s):
  rs = np.random.RandomState(7)
  if kind == "near":                # fronto-parallel plane at ~2.6 m: long runs of equal keys, a few hundred crowded voxels
    return (150.0 + 0.5 * rs.rand(B, 1, H, W)).astype(np.float32)
  n = 1 << s                        # depth log-uniform in 2 .. 195 m, independent per output pixel: no two neighbours share a voxel
  coarse = np.exp(rs.uniform(np.log(2.0), np.log(190.0), (B, 1, H // n + 1, W // n + 1)))
  return np.kron(coarse, np.ones((n, n)))[:, :, :H, :W].astype(np.float32)


def timed(fn, warm=WARM, calls=CALLS, repeats=REPEATS):
  """microseconds per call: (median, min, max) over the repeats"""
  out = []
  for _ in range(repeats):
    for _ in range(warm):
      fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
      fn()
    e1.record()
    torch.cuda.synchronize()
    out.append(e0.elapsed_time(e1) * 1e3 / calls)
  return float(np.median(out)), min(out), max(out)


def fmt(t):
  return "%9.1f [%8.1f .. %8.1f]" % t


def native(proj, disp, rgb):
  def call():
    nat.call("as_disp_to_points", nat.ptr(disp), nat.ptr(rgb), disp.shape[0], H, W, proj.s, ctypes.byref(proj._cam),
             None, None, proj.voxel_size, nat.ptr(proj._table), proj.slots, nat.stream())
    nat.call("as_voxel_cloud_finalize", nat.ptr(proj._table), disp.shape[0], proj.slots, proj.cap, nat.ptr(proj._records),
             nat.ptr(proj._voxel), nat.ptr(proj._count), nat.ptr(proj._n), nat.ptr(proj._dropped), nat.stream())
  return call


def eager(disp, rgb, s):
  """the same pipeline as PyTorch ops on the GPU (float sums, so not bit-reproducible; torch.unique synchronises)"""
  n = 2 ** s
  fb, fxs, fys, cxs, cys = CAM.fx * CAM.baseline, CAM.fx / n, CAM.fy / n, CAM.cx / n, CAM.cy / n
  B = disp.shape[0]
  h, w = H >> s, W >> s
  u = torch.arange(w, device=DEV, dtype=torch.float32).view(1, 1, w)
  v = torch.arange(h, device=DEV, dtype=torch.float32).view(1, h, 1)
  image = torch.arange(B, device=DEV).view(B, 1, 1).expand(B, h, w)

  def call():
    m = disp if s == 0 else F.interpolate(disp, scale_factor=1.0 / n, mode="bilinear", align_corners=False)
    col = rgb if s == 0 else F.interpolate(rgb, scale_factor=1.0 / n, mode="bilinear", align_corners=False)
    depth = torch.clamp(fb / m[:, 0], 0.0, MAX_DEPTH)
    z = (depth * SCALE).to(torch.int32).to(torch.float32) / SCALE
    valid = (z > 0) & (z <= TRUNC)
    xyz = torch.stack([(u - cxs) * z / fxs, (v - cys) * z / fys, z], dim=-1)[valid]
    c = (col.permute(0, 2, 3, 1)[valid] * 255.0).floor()
    # three 20-bit indices below the image number at bit 60: room for |index| < 2^19 and 8 images, enough for the frames timed
    # here (|x| < 80 m / 0.15 m); the product's key holds 21 bits per index and keeps one table per image
    idx = torch.floor(xyz / VOXEL).to(torch.int64) + 2 ** 19
    key = (image[valid] << 60) | (idx[:, 0] << 40) | (idx[:, 1] << 20) | idx[:, 2]
    uniq, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
    acc = torch.zeros(uniq.shape[0], 6, device=DEV).index_add_(0, inv, torch.cat([xyz, c], dim=1))
    return acc / cnt.unsqueeze(1), uniq
  return call


def host(disp, rgb, s):
  def call():
    d, c = disp.cpu().numpy(), rgb.cpu().numpy()
    p = pr.points(d, pr.camera_constants(CAM.fx, CAM.fy, CAM.cx, CAM.cy, CAM.baseline, s), s, MAX_DEPTH, SCALE, TRUNC)
    col = pr.colour_bytes(c, s)
    return [pr.record_bytes(pr.voxel_cloud(p, b, VOXEL, col)) for b in range(d.shape[0])]
  return call


def wall(fn, repeats=REPEATS):
  out = []
  for _ in range(repeats):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    out.append((time.perf_counter() - t0) * 1e6)
  return float(np.median(out)), min(out), max(out)


def forward_per_pair(B):
  from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
  from adaptive_stereo.utils import synthetic as syn
  from train import process_batch
  fnet, snet = FeatureExtractorNetwork(4), StereoNet(4, 1, 0, maxdisp=192)
  fnet.load_state_dict(syn.synthetic_state_dict(fnet.state_dict(), seed=123))
  snet.load_state_dict(syn.synthetic_state_dict(snet.state_dict(), seed=123, logit_gain=20.0))
  fnet, snet = fnet.to(DEV).eval(), snet.to(DEV).eval()
  left, right = (t.to(DEV) for t in syn.stereo_pair(B, H, W, seed=1))
  with torch.no_grad():
    t = timed(lambda: process_batch(fnet, snet, left, right, None))
  return tuple(x / B for x in t)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(HERE, "..", "..", "profiles", "pointcloud_timing.txt"))
  args = ap.parse_args()
  lines = []

  def say(text=""):
    print(text, flush=True)
    lines.append(text)

  say("depth / point-cloud stage at %dx%d, microseconds per call: median [min .. max] of %d repeats of %d calls (%d warm-up)"
      % (H, W, REPEATS, CALLS, WARM))
  say("device: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
  say("native = as_disp_to_points + as_voxel_cloud_finalize (voxel %.2f m); points = valid points inserted, voxels = records out" % VOXEL)
  say()
  say("%-6s %2s %2s %-6s %9s %9s | %-30s" % ("frame", "B", "s", "colour", "points", "voxels", "native"))
  for s in (2, 0):
    for B in (1, 4):
      proj = DepthProjector(H, W, CAM, batch=B, pyramid_scale=s, max_depth=MAX_DEPTH, depth_scale=SCALE, depth_trunc=TRUNC,
                            voxel_size=VOXEL, device=DEV)
      rgb = torch.rand(B, 3, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
      for kind in ("near", "random"):
        disp = torch.from_numpy(frame(kind, B, s)).to(DEV)
        cloud = proj.voxel_cloud(disp, rgb)
        voxels, points = int(cloud.n.sum()), int(sum(int(t["count"].sum()) for t in cloud.trim()))
        assert int(cloud.dropped.sum()) == 0
        for colour in (False, True):
          t = timed(native(proj, disp, rgb if colour else None))
          say("%-6s %2d %2d %-6s %9d %9d | %s" % (kind, B, s, "yes" if colour else "no", points, voxels, fmt(t)))
  say()
  say("the same pipeline elsewhere (with colour): eager PyTorch on the GPU (HIP events; torch.unique synchronises) and the host path")
  say("of the reference's node (.cpu() + numpy, wall clock, %d single calls)" % REPEATS)
  say("%-6s %2s %2s | %-30s | %-30s" % ("frame", "B", "s", "eager PyTorch, GPU", "host (.cpu() + numpy)"))
  for s in (2, 0):
    for B in (1, 4):
      rgb = torch.rand(B, 3, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
      for kind in ("near", "random"):
        disp = torch.from_numpy(frame(kind, B, s)).to(DEV)
        te = timed(eager(disp, rgb, s))
        th = wall(host(disp, rgb, s))
        say("%-6s %2d %2d | %s | %s" % (kind, B, s, fmt(te), fmt(th)))
  say()
  say("for scale: forward-only (train.process_batch, eval mode, k = 4), microseconds per PAIR")
  for B in (1, 4):
    say("B = %d | %s" % (B, fmt(forward_per_pair(B))))
  with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
