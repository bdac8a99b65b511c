"""Times DisparityPainter.paint (csrc/visualize.hip) with HIP events at the two maps a user meets: [4,1,375,1242] (the bench
workload's four KITTI pairs) and [1,1,94,311] (the ROS node's quarter-scale map of one pair) — fixed range (one launch) and
automatic range (two launches), uint8 BGR out.  Beside it, on the host of the same box: the reference's expression for the same
image (device-to-host copy, torch min / max / normalise on the CPU, matplotlib's Colormap.__call__, * 255, cast, channel flip) where
matplotlib is installed; where it is not, the tool says so and times the native path alone.
50 warm-up and 500 timed calls, five repeats (the host path: 2 and 10): median and [min .. max] of the repeats.  There is no
pass/fail time.

usage (GPU box): python tests/tools/time_visualization.py [--out profiles/visualization_timing.txt]
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "adaptive-stereo-icra-2021_amd"))
sys.path.insert(0, os.path.join(HERE, ".."))
import numpy as np
import torch

import visualization_ref as R
from adaptive_stereo.utils import visualization as V

DEV = "cuda:0"
WARM, CALLS, REPEATS = 50, 500, 5
SHAPES = [(4, 1, 375, 1242), (1, 1, 94, 311)]
RANGES = [("fixed 0 .. 115.2", 0, 0.6 * 192), ("automatic", None, None)]


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


def timed_host(fn, warm=2, calls=10, repeats=REPEATS):
  out = []
  for _ in range(repeats):
    for _ in range(warm):
      fn()
    t0 = time.perf_counter()
    for _ in range(calls):
      fn()
    out.append((time.perf_counter() - t0) * 1e6 / calls)
  return float(np.median(out)), min(out), max(out)


def fmt(t):
  return "%9.2f [%8.2f .. %8.2f]" % t


def host_expression(cmap):
  """The reference's visualize_disp_cv per image of the batch, restated with the same library calls."""
  def run(disp, vmin, vmax):
    value = disp.detach().squeeze(1).cpu()
    b, rows, cols = value.shape
    lo, hi = vmin, vmax
    if lo is None:
      lo = torch.min(value.view(b, -1), 1, keepdim=True)[0].unsqueeze(2).expand(-1, rows, cols)
    if hi is None:
      hi = torch.max(value.view(b, -1), 1, keepdim=True)[0].unsqueeze(2).expand(-1, rows, cols)
    mapped = cmap(((value - lo) / (hi - lo)).numpy())
    return np.ascontiguousarray((255.0 * mapped[..., :3]).astype(np.uint8)[..., ::-1])
  return run


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(HERE, "..", "..", "profiles", "visualization_timing.txt"))
  args = ap.parse_args()
  lines = []

  def say(text=""):
    print(text, flush=True)
    lines.append(text)

  try:
    import matplotlib
    host = host_expression(matplotlib.colormaps["inferno"])
    host_note = "matplotlib %s" % matplotlib.__version__
  except ImportError:
    host, host_note = None, "matplotlib is NOT installed on this box: the host column is not measured"
  say("DisparityPainter.paint (uint8 BGR, inferno), microseconds per call: median [min .. max] of %d repeats of %d calls "
      "(%d warm-up), HIP events" % (REPEATS, CALLS, WARM))
  say("device: %s, torch %s; host path: %s" % (torch.cuda.get_device_name(0), torch.__version__, host_note))
  say()
  say("%-18s | %-18s | %-32s | %-32s | %s" % ("[B,1,H,W]", "range", "native paint()", "algorithmic bytes, cache-resident GB/s",
                                            "reference's host expression (wall clock, incl. the copy)"))
  table = V.packaged_colormaps()["inferno"]
  for shape in SHAPES:
    B, _, H, W = shape
    x_host = R.make_case(shape, "plain")
    x = torch.from_numpy(x_host).to(DEV)
    for label, vmin, vmax in RANGES:
      painter = V.DisparityPainter(H, W, batch=B, cmap="inferno", vmin=vmin, vmax=vmax, order="bgr", device=DEV)
      # agreement first: a timing of something that computes another result is worth nothing
      want = R.paint_u8(table, R.index(x_host, vmin, vmax), "bgr")
      assert np.array_equal(painter.paint(x).cpu().numpy(), want)
      if host is not None:
        assert np.array_equal(host(x, vmin, vmax), want)
      t = timed(lambda: painter.paint(x))
      nbytes = B * H * W * ((4 if vmin is not None and vmax is not None else 8) + 3)
      say("%-18s | %-18s | %-32s | %8.2f MB, %7.1f GB/s          | %s"
          % (list(shape), label, fmt(t), nbytes / 1e6, nbytes / t[0] / 1e3,
             fmt(timed_host(lambda: host(x, vmin, vmax))) if host is not None else "not measured"))
  say()
  say("native: as_colormap_apply alone (fixed) or as_colormap_range + as_colormap_apply (automatic), launches back to back on one")
  say("stream, so the figure includes launch overhead; the maps are a few MB, so these launches are latency-bound, not HBM-bound.")
  say("The GB/s column is algorithmic bytes / median time with the SAME few-MB input read on every call: it stays resident in the")
  say("256 MB last-level cache, so the column is a cache-resident rate and NOT an HBM rate.")
  with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
