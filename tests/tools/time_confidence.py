"""Times the three entry points behind adaptive_stereo.confidence with device events, warm.

  python tests/tools/time_confidence.py [--out FILE] [--rounds N]

  as_disp_confidence        logits 4 x 12 x 24 x 78 (the bench workload's coarse volume), all three maps
  as_sparsification         4 x 375 x 1242 elements, 256 bins, a uniform key
  as_disp_to_points_gated   4 x 375 x 1242, s = 2, with a table, against as_disp_to_points in the same run: the two alternate, one
                            block of launches each per round, so the spread over the rounds is seen beside their difference.  Each
                            launch is followed by its as_voxel_cloud_finalize (the table has to be handed back empty); the pair
                            is what is timed, for both.
Every figure is the mean over a block of back-to-back launches between two device events; per entry point the rounds' minimum,
median and maximum are printed.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "adaptive-stereo-icra-2021_amd"))
import torch

from adaptive_stereo import _native as nat
from adaptive_stereo.pointcloud import DepthProjector, StereoCamera


def timed(fn, warm=10, reps=200):
  for _ in range(warm):
    fn()
  torch.cuda.synchronize()
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(reps):
    fn()
  stop.record()
  torch.cuda.synchronize()
  return start.elapsed_time(stop) * 1e3 / reps            # microseconds per call


def summary(values):
  return dict(min_us=min(values), median_us=statistics.median(values), max_us=max(values), rounds=len(values))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--rounds", type=int, default=7)
  opt = ap.parse_args()
  assert torch.cuda.is_available(), "needs a GPU"
  dev = "cuda:0"
  g = torch.Generator(device=dev).manual_seed(1)
  rows = {}

  B, D, Hc, Wc = 4, 12, 24, 78
  logits = torch.randn(B, D, Hc, Wc, device=dev, generator=g) * 5.0
  maps = [torch.empty(B, Hc, Wc, device=dev) for _ in range(3)]

  def confidence():
    nat.call("as_disp_confidence", nat.ptr(logits), B, D, Hc, Wc, nat.ptr(maps[0]), nat.ptr(maps[1]), nat.ptr(maps[2]), nat.stream())
  rows["as_disp_confidence 4x12x24x78"] = summary([timed(confidence) for _ in range(opt.rounds)])

  H, W, K = 375, 1242, 256
  n = B * H * W
  key = torch.rand(n, device=dev, generator=g)
  gt = torch.rand(n, device=dev, generator=g) * 60.0 + 1.0
  pred = gt + torch.randn(n, device=dev, generator=g) * 3.0
  ints = torch.zeros(2 * K + 1, dtype=torch.int64, device=dev)
  err = torch.zeros(K, dtype=torch.float64, device=dev)

  def bins():
    nat.call("as_sparsification", nat.ptr(key), nat.ptr(pred), nat.ptr(gt), n, 0.0, float(K), K, 3.0, nat.ptr(ints),
             nat.c_vp(ints.data_ptr() + 8 * K), nat.ptr(err), nat.c_vp(ints.data_ptr() + 16 * K), nat.stream())
  rows["as_sparsification 4x375x1242 K=256"] = summary([timed(bins) for _ in range(opt.rounds)])
  rows["as_sparsification 4x375x1242 K=256"]["bytes"] = 12 * n

  s = 2
  cam = StereoCamera(721.5, 721.5, 609.6, 172.9, 0.54)
  proj = DepthProjector(H, W, cam, batch=B, pyramid_scale=s, device=dev)
  disp = torch.rand(B, 1, H, W, device=dev, generator=g) * 180.0 + 4.0
  rgb = torch.rand(B, 3, H, W, device=dev, generator=g)
  conf = torch.rand(B, H >> s, W >> s, device=dev, generator=g)

  def finalize():
    nat.call("as_voxel_cloud_finalize", nat.ptr(proj._table), B, proj.slots, proj.cap, nat.ptr(proj._records), nat.ptr(proj._voxel),
             nat.ptr(proj._count), nat.ptr(proj._n), nat.ptr(proj._dropped), nat.stream())

  def plain():
    nat.call("as_disp_to_points", nat.ptr(disp), nat.ptr(rgb), B, H, W, s, ctypes.byref(proj._cam), None, None, proj.voxel_size,
             nat.ptr(proj._table), proj.slots, nat.stream())
    finalize()

  def gated(conf_min, count=True):
    def run():
      nat.call("as_disp_to_points_gated", nat.ptr(disp), nat.ptr(rgb), nat.ptr(conf), conf_min, B, H, W, s, ctypes.byref(proj._cam),
               None, None, proj.voxel_size, nat.ptr(proj._table), proj.slots, nat.ptr(proj._rejected) if count else None, nat.stream())
      finalize()
    return run
  legs = {"as_disp_to_points + finalize": plain, "as_disp_to_points_gated(-inf) + finalize": gated(float("-inf")),
          "as_disp_to_points_gated(-inf, rejected = NULL) + finalize": gated(float("-inf"), False),
          "as_disp_to_points_gated(0.5) + finalize": gated(0.5), "as_voxel_cloud_finalize alone (empty table)": finalize}
  times = {name: [] for name in legs}
  for _ in range(opt.rounds):                              # alternating: every round times each leg once
    for name, fn in legs.items():
      times[name].append(timed(fn))
  for name, v in times.items():
    rows[name + " 4x375x1242 s=2"] = summary(v)
  rows["what"] = "device events around 200 back-to-back calls after 10 warm-up calls; %d rounds, the legs of the point cloud alternating" % opt.rounds
  for name, r in rows.items():
    print(name, json.dumps(r))
  if opt.out:
    with open(opt.out, "w") as f:
      json.dump(rows, f, indent=1, sort_keys=True)
      f.write("\n")


if __name__ == "__main__":
  sys.exit(main())
