"""Times the entry points behind adaptive_stereo.sgm with device events, warm, at 4 x 375 x 1242, D = 192.

  python tests/tools/time_sgm.py [--out_dir DIR] [--rounds N] [--reps N] [--skip_network]

  (a) as_sgm_census            one image batch, C = 3
  (b) as_sgm_aggregate         at 4 and at 8 paths (3 and 7 launches)
  (c) as_sgm_select            both views, every output
  (d) SemiGlobalMatcher        the whole call: two census launches, the aggregation, the selection
  (e) ProxyLabeler replayed    matcher, left-right check, speckle filter, labels: one graph replay, as a share of
      BothViewInference replayed, the network's own both-view pass on the same box in the same run
Within a group the legs alternate, one block of launches each per round, so the spread over the rounds is seen beside their
difference.  Every figure is the mean over a block of --reps back-to-back calls between two device events after 3 warm-up calls;
per leg the rounds' minimum, median and maximum, the algorithmic bytes per call (every pass over a tensor the launches need, see
`bytes_of`) and what the median makes of them in GB/s, also as a share of the HBM rate a float4 copy reaches on an MI355X
(6.29 TB/s of the 8 TB/s of the specification).  Writes sgm_timing.json and sgm_timing.txt into --out_dir (default: profiles/).
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(REPO, "adaptive-stereo-icra-2021_amd"))
import torch

from adaptive_stereo import _native as nat
from adaptive_stereo import consistency as cons
from adaptive_stereo import sgm

HBM_MEASURED_GBPS = 6290.0            # what a float4 copy reaches on an MI355X: 79 % of the 8 TB/s of the specification


def timed(fn, warm, reps):
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


def summary(values, nbytes=None, launches=None):
  row = dict(min_us=min(values), median_us=statistics.median(values), max_us=max(values), rounds=len(values))
  if launches is not None:
    row["launches"] = launches
  if nbytes is not None:
    row["bytes"] = nbytes
    row["median_GBps"] = nbytes / row["median_us"] * 1e-3
    row["share_of_measured_HBM_rate"] = row["median_GBps"] / HBM_MEASURED_GBPS
  return row


def alternate(legs, rounds, reps):
  times = {name: [] for name in legs}
  for _ in range(rounds):
    for name, fn in legs.items():
      times[name].append(timed(fn, 3, reps))
  return times


def bytes_of(B, C, H, W, D):
  """algorithmic bytes per call.  census: the image in, the words out.  aggregation: the row launch writes S and then reads and
  writes it again (3 passes), every further direction reads and writes it once (2 passes), each launch reads both census maps.
  selection: S once (the right view's diagonal is the same bytes), the four maps and the counts out."""
  n, vol = B * H * W, B * H * W * D * 2
  agg = lambda launches: (3 + 2 * (launches - 1)) * vol + launches * 2 * n * 8
  return {"census": n * (C * 4 + 8), "aggregate4": agg(3), "aggregate8": agg(7), "select": vol + n * 10 + B * 64}


def scene(B, C, H, W, dev, seed):
  """a textured pair with a known RIGHT-view disparity: a ground plane of 5 .. 60 with two boxes in front of it, the right view
  gathered from the left one, right[x] = left[x + d_r(x)] (noise where that leaves the image)"""
  g = torch.Generator(device=dev).manual_seed(seed)
  left = torch.rand(B, C, H, W, device=dev, generator=g)
  y = torch.arange(H, device=dev).view(1, 1, H, 1)
  disp = (5 + 55 * y // H).expand(B, 1, H, W).clone()
  disp[:, :, 100:250, 400:700] = 90
  disp[:, :, 40:90, 900:1100] = 40
  source = torch.arange(W, device=dev).view(1, 1, 1, W) + disp
  inside = source < W
  right = torch.gather(left, -1, source.clamp(max=W - 1).expand(B, C, H, W))
  right = torch.where(inside, right, torch.rand(B, C, H, W, device=dev, generator=g))
  return left.contiguous(), right.contiguous(), disp.float(), inside


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out_dir", default=os.path.join(REPO, "profiles"))
  ap.add_argument("--rounds", type=int, default=5)
  ap.add_argument("--reps", type=int, default=20)
  ap.add_argument("--skip_network", action="store_true", help="leave out BothViewInference in (e)")
  opt = ap.parse_args()
  assert torch.cuda.is_available(), "needs a GPU"
  dev = "cuda:0"
  B, C, H, W, D = 4, 3, 375, 1242, 192
  shape = "%dx%dx%d D=%d" % (B, H, W, D)
  nb = bytes_of(B, C, H, W, D)
  left, right, truth, inside = scene(B, C, H, W, dev, 1)
  notes, rows = [], {}

  m8 = sgm.SemiGlobalMatcher(H, W, batch=B, maxdisp=D, paths=8, channels=C, device=dev)
  res = m8(left, right)
  kept = (res.code_r == 0) & inside
  err = (res.disp_r - truth).abs()[kept]
  notes.append("scene: share of each code, image 0, left view %s, right view %s; of the kept right-view pixels %.4f lie within 1 px "
               "of the scene's disparity" % (m8.fractions()[0, 0].round(4).tolist(), m8.fractions()[0, 1].round(4).tolist(),
                                      float((err <= 1).float().mean())))
  cl, cr, vol, r = m8.census(left), m8.census(right, right=True), m8.volume(), m8.result()
  st = nat.stream

  def aggregate(paths):
    return lambda: nat.call("as_sgm_aggregate", nat.ptr(cl), nat.ptr(cr), B, H, W, D, 10, 120, paths, nat.ptr(vol), st())
  legs = {"(a) as_sgm_census": lambda: m8.census(left),
          "(b) as_sgm_aggregate, 4 paths": aggregate(4), "(b) as_sgm_aggregate, 8 paths": aggregate(8),
          "(c) as_sgm_select, both views, every output": lambda: nat.call(
              "as_sgm_select", nat.ptr(vol), B, H, W, D, 5, float("nan"), nat.ptr(r.disp_l), nat.ptr(r.code_l), nat.ptr(r.disp_r),
              nat.ptr(r.code_r), nat.ptr(r.counts), st()),
          "(d) SemiGlobalMatcher, the whole call, 8 paths": lambda: m8(left, right)}
  meta = {"(a) as_sgm_census": (nb["census"], 1), "(b) as_sgm_aggregate, 4 paths": (nb["aggregate4"], 3),
          "(b) as_sgm_aggregate, 8 paths": (nb["aggregate8"], 7), "(c) as_sgm_select, both views, every output": (nb["select"], 2),
          "(d) SemiGlobalMatcher, the whole call, 8 paths": (2 * nb["census"] + nb["aggregate8"] + nb["select"], 11)}
  for name, v in alternate(legs, opt.rounds, opt.reps).items():
    rows["%s %s" % (name, shape)] = summary(v, *meta[name])

  lab = sgm.ProxyLabeler(H, W, batch=B, maxdisp=D, channels=C, device=dev).capture(left, right)
  labels, code, counts = lab(left, right)
  notes.append("proxy labels: share of each final code, image 0: %s; labels on %.4f of the pixels"
               % ([round(int(c) / float(H * W), 4) for c in counts[0].cpu()], float((labels > 0).float().mean())))
  legs = {"(e) ProxyLabeler, one graph replay": lambda: lab(left, right)}
  if not opt.skip_network:
    from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
    from adaptive_stereo.utils import synthetic as syn
    k = 4
    fnet, snet = FeatureExtractorNetwork(k), StereoNet(k, 1, 0, maxdisp=192)
    fnet.load_state_dict(syn.synthetic_state_dict(fnet.state_dict(), seed=123))
    snet.load_state_dict(syn.synthetic_state_dict(snet.state_dict(), seed=123, logit_gain=20.0))
    fnet, snet = fnet.to(dev).eval(), snet.to(dev).eval()
    both = cons.BothViewInference(fnet, snet, H, W, batch=B).capture(left, right)
    legs["(e) BothViewInference k=4, one graph replay"] = lambda: both(left, right)
  for name, v in alternate(legs, opt.rounds, opt.reps).items():
    rows["%s %s" % (name, shape)] = summary(v)
  if not opt.skip_network:
    a, b = (rows["%s %s" % (name, shape)]["median_us"] for name in legs)
    rows["(e) ProxyLabeler as a share of BothViewInference"] = a / b

  what = ("device events around %d back-to-back calls after 3 warm-up calls; %d rounds, the legs of a group alternating; microseconds "
          "per call; bytes are algorithmic (tests/tools/time_sgm.py bytes_of), GB/s is bytes over the median, the share is that over "
          "%.0f GB/s" % (opt.reps, opt.rounds, HBM_MEASURED_GBPS))
  lines = ["as_sgm_census, as_sgm_aggregate, as_sgm_select (csrc/sgm.hip) and adaptive_stereo.sgm on one MI355X,",
           "python tests/tools/time_sgm.py: " + what + "."] + notes + [""]
  lines.append("%-62s %10s %10s %10s %9s %13s %7s %6s" % ("leg, " + shape, "min", "median", "max", "launches", "bytes", "GB/s", "share"))
  for name, row in rows.items():
    if not isinstance(row, dict):
      lines.append("%-62s %10.4f" % (name, row))
      continue
    tail = "%9s %13s %7s %6s" % (row.get("launches", ""), row.get("bytes", ""),
                                 "%.0f" % row["median_GBps"] if "bytes" in row else "",
                                 "%.3f" % row["share_of_measured_HBM_rate"] if "bytes" in row else "")
    lines.append("%-62s %10.1f %10.1f %10.1f %s" % (name.replace(" " + shape, ""), row["min_us"], row["median_us"], row["max_us"], tail))
  text = "\n".join(lines) + "\n"
  print(text)
  rows["what"], rows["notes"] = what, notes
  os.makedirs(opt.out_dir, exist_ok=True)
  with open(os.path.join(opt.out_dir, "sgm_timing.json"), "w") as f:
    json.dump(rows, f, indent=1, sort_keys=True)
    f.write("\n")
  with open(os.path.join(opt.out_dir, "sgm_timing.txt"), "w") as f:
    f.write(text)


if __name__ == "__main__":
  sys.exit(main())
