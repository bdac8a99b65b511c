"""Times adaptive_stereo.smooth.DisparitySmoother as captured-graph replays at 4 x 375 x 1242, beside the two floors of
csrc/disp_smooth.hip that DESIGN.md states.

  python tests/tools/time_disp_smooth.py [--out FILE] [--rounds N]

Three settings: radius 1 unguided, radius 3 guided, radius 7 guided (three guide planes, sigma_color 0.1, no fill, no code_in), on
the smooth scene of time_disp_filter.py (a ground plane, boxes, islands, holes) and a guide that shares its edges.  Each setting is
captured once (capture.warm_up_and_capture); a figure is the mean over a block of 100 replays between two device events after 10
warm-up replays; the settings alternate, one block each per round, and per setting the rounds' minimum, median and maximum are
printed.
The floors per setting, from the kernel's own scheme:
  HBM   bytes read and written once per pixel: disp 4, out 4, code 1, and 4 per guide plane
  LDS   (1 + passes) x taps x (1 word unguided, 3 guided: key, guide, table entry) 4-byte reads per pixel, `passes` being the mean
        number of bisection passes, counted by a numpy emulation of the kernel's selection on a 48 x 160 crop of the same scene;
        the plain median at radius 1 and 2 (the register sorting network) reads its taps once
against 6.29 TB/s of HBM (measured copy rate) and 75 TB/s of 4-byte LDS reads over all CUs.
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "adaptive-stereo-icra-2021_amd"))
sys.path.insert(0, os.path.join(HERE, ".."))
import numpy as np
import torch

import disp_smooth_ref as ds
from adaptive_stereo import capture
from adaptive_stereo import smooth
from time_disp_filter import scenes

HBM_BYTES_PER_S = 6.29e12
LDS_READS_PER_S = 75e12 / 4
SETTINGS = [("radius 1, unguided", 1, None), ("radius 3, guided", 3, 0.1), ("radius 7, guided", 7, 0.1)]


def mean_passes(disp, guide, lut, radius):
  """the kernel's selection, emulated: the mean number of passes after pass 0 over the usable pixels of disp [1,1,h,w]"""
  us = ds.usable(disp)
  key = ds.keys(disp).astype(np.int64)
  g = None if guide is None else ds.quantise(guide)
  taps, weights = [], []
  for dy in range(-radius, radius + 1):
    for dx in range(-radius, radius + 1):
      on = ds._shifted(us, dy, dx, False)
      taps.append(np.where(on, ds._shifted(key, dy, dx, 0), ds.NOT_A_TAP))
      w = 1 if g is None else np.clip(lut, 0, 65535)[np.abs(g - ds._shifted(g, dy, dx, 0)).sum(axis=1, keepdims=True)]
      weights.append(np.where(on, w, 0))
  taps, weights = np.stack(taps), np.stack(weights)
  wt = weights.sum(axis=0)
  lo = taps.min(axis=0)
  hi = np.where(taps == ds.NOT_A_TAP, -(1 << 40), taps).max(axis=0)
  hi = np.where(us & (wt > 0), hi, lo)
  passes = np.zeros(lo.shape, dtype=np.int64)
  while (lo < hi).any():
    live = lo < hi
    t = lo + (hi - lo) // 2
    le = taps <= t
    cum = np.where(le, weights, 0).sum(axis=0)
    below = np.where(le, taps, -(1 << 40)).max(axis=0)
    above = np.where(le, 1 << 41, taps).min(axis=0)
    down = 2 * cum >= wt
    hi = np.where(live & down, below, hi)
    lo = np.where(live & ~down, above, lo)
    passes += live
  want = ds.wmedian(disp, None, guide, lut, radius)["out"]
  assert np.array_equal(ds.keys(want)[us], lo[us].astype(np.int32)), "the emulated selection is the restatement's"
  return float(passes[us].mean())


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--rounds", type=int, default=7)
  opt = ap.parse_args()
  assert torch.cuda.is_available(), "needs a GPU"
  dev = "cuda:0"
  gen = torch.Generator(device=dev).manual_seed(1)
  B, H, W = 4, 375, 1242
  n = B * H * W
  _, scene = scenes(B, H, W, dev, gen)
  base = torch.nan_to_num(scene, nan=0.0) / 110.0
  guide = (base + 0.02 * torch.rand(B, 3, H, W, device=dev, generator=gen)).clamp(0, 1).contiguous()

  rows, replays = {}, {}
  crop = (slice(0, 1), slice(None), slice(90, 138), slice(380, 540))                  # across the edge of a box
  for name, radius, sigma in SETTINGS:
    sm = smooth.DisparitySmoother(H, W, batch=B, radius=radius, sigma_color=sigma, device=dev)
    g = guide if sigma is not None else None
    run = lambda sm=sm, g=g: sm(scene, g)
    graph, result = capture.warm_up_and_capture(run, 2, run)
    graph.replay()
    torch.cuda.synchronize()
    shares = sm.fractions()[0].round(4).tolist()
    host_guide = None if g is None else g[crop].cpu().numpy()
    passes = mean_passes(scene[crop].cpu().numpy(), host_guide, None if g is None else sm.weight_table(), radius)
    taps = (2 * radius + 1) ** 2
    hbm_bytes = 9 + (12 if g is not None else 0)
    network = g is None and radius <= 2
    lds_reads = taps if network else (1 + passes) * taps * (3 if g is not None else 1)
    rows[name] = dict(shares_image0=shares, mean_passes=None if network else passes, hbm_bytes_per_pixel=hbm_bytes, lds_reads_per_pixel=lds_reads,
                      hbm_floor_us=n * hbm_bytes / HBM_BYTES_PER_S * 1e6, lds_floor_us=n * lds_reads / LDS_READS_PER_S * 1e6)
    replays[name] = graph

  def timed(graph, warm=10, reps=100):
    for _ in range(warm):
      graph.replay()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
      graph.replay()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps                       # microseconds per replay

  times = {name: [] for name in replays}
  for _ in range(opt.rounds):
    for name, graph in replays.items():
      times[name].append(timed(graph))
  for name, v in times.items():
    r = rows[name]
    r.update(min_us=min(v), median_us=statistics.median(v), max_us=max(v), rounds=len(v))
    floor = max(r["hbm_floor_us"], r["lds_floor_us"])
    r["larger_floor"] = "LDS" if r["lds_floor_us"] >= r["hbm_floor_us"] else "HBM"
    r["floor_over_median"] = floor / r["median_us"]
  rows["what"] = ("captured-graph replays of DisparitySmoother at %dx%dx%d (the clearing launch and the kernel): device events "
                  "around 100 replays after 10 warm-up replays; %d rounds, the settings alternating" % (B, H, W, opt.rounds))
  for name, r in rows.items():
    print(name, json.dumps(r))
  if opt.out:
    with open(opt.out, "w") as f:
      json.dump(rows, f, indent=1, sort_keys=True)
      f.write("\n")


if __name__ == "__main__":
  sys.exit(main())
