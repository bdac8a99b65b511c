"""Times as_cost_volume_probe (csrc/cv_probe.hip) with HIP events at two coarse volumes a user meets: [4,12,24,78] (the bench
workload, k = 4 at 375x1242, four pairs) and [4,24,47,156] (k = 3 at the same size) — what CostVolumeProbe.add launches (the cursor
launch included), without and with the rank profile.  Beside it, in the same process on the same device:
  * as_fcs_scores, scores only (FcsCollector.add): the launch the probe is expected to cost about as much as;
  * what a user composes without the probe: ood.fcs_scores(maps=True), torch.argmax / argmin per image, the gather of the two
    slices, torch.sort, and the read-backs of row, col, max, mean and gt per image (each a synchronisation).
50 warm-up and 500 timed calls, five repeats: median and [min .. max] of the repeats; the composed path is also timed with the
host clock around a final synchronise, since its read-backs stall the host.  There is no pass/fail time.

usage (GPU box): python tests/tools/time_cv_probe.py [--out profiles/cv_probe_timing.txt]
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "adaptive-stereo-icra-2021_amd"))
import numpy as np
import torch

from adaptive_stereo import _native as nat
from adaptive_stereo import cv_probe, ood

DEV = "cuda:0"
WARM, CALLS, REPEATS = 50, 500, 5
SHAPES = [(4, 12, 24, 78), (4, 24, 47, 156)]


def timed(fn, warm=WARM, calls=CALLS, repeats=REPEATS):
  """microseconds per call by HIP events and by the host clock: two (median, min, max) over the repeats"""
  dev, host = [], []
  for _ in range(repeats):
    for _ in range(warm):
      fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
      fn()
    e1.record()
    torch.cuda.synchronize()
    host.append((time.perf_counter() - t0) * 1e6 / calls)
    dev.append(e0.elapsed_time(e1) * 1e3 / calls)
  return (float(np.median(dev)), min(dev), max(dev)), (float(np.median(host)), min(host), max(host))


def fmt(t):
  return "%8.2f [%7.2f .. %7.2f]" % t


def composed(x, gt):
  """The same numbers without the probe: per image two picks, two slices, their sorted values, read back one by one."""
  scores, fmean, _ = ood.fcs_scores(x, maps=True)
  out = []
  W = x.shape[-1]
  for b in range(x.shape[0]):
    flat = fmean[b].flatten()
    for arg in (torch.argmax, torch.argmin):
      idx = arg(flat)
      row, col = idx // W, idx % W
      curve = x[b, :, row, col]
      srt = torch.sort(curve, descending=True)[0]
      out.append((row.item(), col.item(), srt[0].item(), srt[2:].mean().item(), gt[b, 0, row, col].item(), curve))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(HERE, "..", "..", "profiles", "cv_probe_timing.txt"))
  args = ap.parse_args()
  lines = []

  def say(text=""):
    print(text, flush=True)
    lines.append(text)

  say("as_cost_volume_probe against as_fcs_scores and against the composed torch path, microseconds per call: median "
      "[min .. max] of %d repeats of %d calls (%d warm-up)" % (REPEATS, CALLS, WARM))
  say("device: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
  for shape in SHAPES:
    B, D, H, W = shape
    x = torch.randn(*shape, device=DEV, generator=torch.Generator(DEV).manual_seed(5)) * 20.0
    gt = torch.rand(B, 1, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(6)) * D
    plain = cv_probe.CostVolumeProbe(B, D, profile=False, device=DEV)
    ranked = cv_probe.CostVolumeProbe(B, D, profile=True, device=DEV)
    fcs = ood.FcsCollector(B, device=DEV)

    # agreement first: a timing of something that computes another result is worth nothing
    ranked.add(x, gt)
    res = ranked.results().cpu()
    for i, (row, col, mx, mean, g, curve) in enumerate(composed(x, gt)):
      b, which = divmod(i, 2)
      assert (int(res.row[b, which]), int(res.col[b, which])) == (row, col)
      assert float(res.max[b, which]) == mx and float(res.gt[b, which]) == g
      assert abs(float(res.mean_rest[b, which]) - mean) <= 1e-4 * max(1.0, abs(mean))
      assert torch.equal(res.slices[b, which], curve.cpu())

    # a row past the capacity is skipped before its image is read, so a collector that has filled up would time an empty
    # launch: the timed calls go to the entry point without a cursor (rows 0 .. B-1 every time) but with the dropped counter,
    # which keeps the second, one-lane launch in
    def probe(col):
      nat.call("as_cost_volume_probe", nat.ptr(x), nat.ptr(gt), B, D, H, W, nat.ptr(col._pix), nat.ptr(col._vals),
               nat.ptr(col._slices), nat.ptr(col._profile), B, None, nat.ptr(col._dropped), nat.stream())

    rows = [("as_fcs_scores, scores only (+cursor)", timed(lambda: fcs.add(x))),
            ("probe without the profile (+cursor launch)", timed(lambda: probe(plain))),
            ("probe with the profile (+cursor launch)", timed(lambda: probe(ranked))),
            ("composed: fcs_scores(maps) + argmax/argmin + gather + sort + %d read-backs" % (10 * B),
             timed(lambda: composed(x, gt), warm=5, calls=50))]
    say()
    say("%s" % (list(shape),))
    say("  %-78s | %-28s | %-28s" % ("", "HIP events", "host clock incl. final sync"))
    for name, (dev, host) in rows:
      say("  %-78s | %s | %s" % (name, fmt(dev), fmt(host)))
    say("  the profile costs %.2fx the launch without it; the probe without it costs %.2fx as_fcs_scores" % (
        rows[2][1][0][0] / rows[1][1][0][0], rows[1][1][0][0] / rows[0][1][0][0]))
  with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
