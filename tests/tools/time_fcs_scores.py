"""Times as_fcs_scores (csrc/ood.hip) with HIP events at the two coarse volumes a user meets: [4,12,24,78] (the bench workload,
k = 4 at 375x1242, four pairs) and [1,24,68,120] (k = 3 at 540x960, one pair) — scores only (what FcsCollector.add launches,
cursor included) and scores with both maps.  Beside it, in the same process on the same device: the reference's expression for
the same result as torch ops (sort, max, median, mean(dim=(-2,-1)); utils/feature_contrast.py and ood_analysis.py:76-77).
50 warm-up and 500 timed calls, five repeats: median and [min .. max] of the repeats.  There is no pass/fail time.

usage (GPU box): python tests/tools/time_fcs_scores.py [--out profiles/fcs_scores_timing.txt]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "adaptive-stereo-icra-2021_amd"))
import numpy as np
import torch

from adaptive_stereo import _native as nat
from adaptive_stereo import ood

DEV = "cuda:0"
WARM, CALLS, REPEATS = 50, 500, 5
SHAPES = [(4, 12, 24, 78), (1, 24, 68, 120)]


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
  return "%8.2f [%7.2f .. %7.2f]" % t


def torch_scores(x):
  """the reference's two functions and its per-image mean, as torch ops"""
  srt = torch.sort(x, dim=1, descending=True)[0]
  fmean = srt[:, 0] - srt[:, 2:].mean(dim=1)
  fmed = torch.max(x, dim=1)[0] - torch.median(x, dim=1)[0]
  return torch.stack([fmean.mean(dim=(-2, -1)), fmed.mean(dim=(-2, -1))], dim=1), fmean, fmed


def torch_mean_score_only(x):
  """what ood_analysis.py:76-77 runs per batch (without its .cpu())"""
  srt = torch.sort(x, dim=1, descending=True)[0]
  return (srt[:, 0] - srt[:, 2:].mean(dim=1)).mean(dim=(-2, -1))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(HERE, "..", "..", "profiles", "fcs_scores_timing.txt"))
  args = ap.parse_args()
  lines = []

  def say(text=""):
    print(text, flush=True)
    lines.append(text)

  say("as_fcs_scores against the reference's torch expression, microseconds per call: median [min .. max] of %d repeats of %d "
      "calls (%d warm-up), HIP events" % (REPEATS, CALLS, WARM))
  say("device: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
  say()
  say("%-16s | %-28s | %-28s | %-28s | %-28s" % ("[B,D,H,W]", "native, scores only (+cursor)", "native, scores + both maps",
                                                 "torch, both scores + maps", "torch, mean score only"))
  for shape in SHAPES:
    B, D, H, W = shape
    x = torch.randn(*shape, device=DEV, generator=torch.Generator(DEV).manual_seed(5)) * 20.0
    col = ood.FcsCollector(B, device=DEV)
    scores = torch.empty(B, 2, device=DEV)
    fm, fd = torch.empty(B, H, W, device=DEV), torch.empty(B, H, W, device=DEV)

    def collector_add():
      col.add(x)

    def both_maps():
      nat.call("as_fcs_scores", nat.ptr(x), B, D, H, W, nat.ptr(fm), nat.ptr(fd), nat.ptr(scores), B, None, None, nat.stream())

    # agreement first: a timing of something that computes another result is worth nothing
    both_maps()
    ts, tm, td = torch_scores(x)
    assert torch.equal(fd, td) and float((fm - tm).abs().max()) <= 1e-3
    assert float((scores - ts).abs().max()) <= 1e-4 * float(ts.abs().max())
    t = [timed(collector_add), timed(both_maps), timed(lambda: torch_scores(x)), timed(lambda: torch_mean_score_only(x))]
    say("%-16s | %s | %s | %s | %s" % (list(shape), fmt(t[0]), fmt(t[1]), fmt(t[2]), fmt(t[3])))
  say()
  say("native scores only = FcsCollector.add: fcs_scores_kernel (one workgroup per image) + the one-lane cursor launch; rows past")
  say("the capacity are dropped, which costs the same.  The torch columns allocate their intermediates from the caching allocator.")
  with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
