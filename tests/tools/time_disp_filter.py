"""Times the entry points behind adaptive_stereo.disp_filter with device events, warm, at 4 x 375 x 1242.

  python tests/tools/time_disp_filter.py [--out FILE] [--rounds N] [--skip_network] [--skip_host]

  (a) as_disp_edge_check       all four outputs and the code only, against (c)
  (c) torch composition        the edge check's contract from stock operators (pad, where, maximum), first compared for equality
  (b) as_disp_speckle          on the scene of time_lr_consistency.py plus planted islands (per-row levels: components are runs of
                               a row), on a smooth scene (a ground plane, boxes, islands, holes: components are regions), and on
                               what the edge check kept of the smooth scene (DisparityFilter.__call__, both stages)
  (x) adversarial maps         one component covering every image (one root, the contended counter) and the checkerboard of
                               usable pixels (every pixel a root)
  (h) the host route           what a caller has today: copy to the host, scipy.ndimage.label + bincount (max_diff = +inf), copy
                               back; wall clock around a synchronised call
  (d) FilteredBothViewInference replayed against BothViewInference replayed: the stage as a share of the forward pass
Within a group the legs alternate, one block of launches each per round, so the spread over the rounds is seen beside their
difference.  Every device figure is the mean over a block of 200 back-to-back calls between two device events after 10 warm-up
calls; per leg the rounds' minimum, median and maximum are printed, and for the kernels the algorithmic bytes (every tensor read
once and written once) and what the median makes of them in GB/s.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "adaptive-stereo-icra-2021_amd"))
import torch

from adaptive_stereo import _native as nat
from adaptive_stereo import consistency as cons
from adaptive_stereo import disp_filter as dfm


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


def wall(fn, reps=3):
  fn()
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(reps):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e6 / reps


def summary(values, nbytes=None):
  row = dict(min_us=min(values), median_us=statistics.median(values), max_us=max(values), rounds=len(values))
  if nbytes is not None:
    row["bytes"] = nbytes
    row["median_GBps"] = nbytes / row["median_us"] * 1e-3
  return row


def alternate(legs, rounds, clock=timed):
  times = {name: [] for name in legs}
  for _ in range(rounds):
    for name, fn in legs.items():
      times[name].append(clock(fn))
  return times


def torch_edge(D, tol_abs, tol_rel):
  """as_disp_edge_check's contract without code_in, all four outputs, from stock operators"""
  nan = float("nan")
  us = (D >= 0) & ~torch.isinf(D)
  tol = torch.clamp(tol_rel * D, min=tol_abs)
  P = torch.nn.functional.pad(D, (1, 1, 1, 1), value=nan)
  H, W = D.shape[-2:]
  jump = torch.zeros_like(D)
  over = torch.zeros_like(us)
  for dy, dx in ((1, 0), (1, 2), (0, 1), (2, 1)):
    dq = P[..., dy:dy + H, dx:dx + W]
    usq = (dq >= 0) & ~torch.isinf(dq)
    e = (D - dq).abs()
    jump = torch.where(usq, torch.maximum(jump, e), jump)
    over |= usq & (e > tol)
  code = torch.where(us, torch.where(over, 5, 0), 4).to(torch.uint8)
  counts = torch.stack([(code == k).flatten(1).sum(1) for k in range(7)], 1).int()
  return code, (code == 0).float(), torch.where(us, jump, torch.full((), nan, device=D.device)), counts


def scenes(B, H, W, dev, g):
  """the check's scene of time_lr_consistency.py and a smooth one, both with planted islands and holes"""
  rows = 20.0 + 10.0 * torch.rand(B, 1, H, 1, device=dev, generator=g) + torch.rand(B, 1, H, W, device=dev, generator=g)
  rows[:, :, 100:250, 400:700] += 30.0
  y = torch.arange(H, device=dev, dtype=torch.float32).view(1, 1, H, 1)
  smooth = 5.0 + 60.0 * y / H + 0.2 * torch.rand(B, 1, H, W, device=dev, generator=g)
  smooth[:, :, 100:250, 400:700] += 30.0
  smooth[:, :, 40:90, 900:1100] += 12.0
  cpu = torch.Generator().manual_seed(2)
  for m in (rows, smooth):
    for _ in range(300):                                  # islands of 2 .. 12 pixels a side, 8 above their surroundings
      b, y0, x0 = (int(torch.randint(0, n, (1,), generator=cpu)) for n in (B, H - 12, W - 12))
      h, w = (int(torch.randint(2, 13, (1,), generator=cpu)) for _ in range(2))
      m[b, :, y0:y0 + h, x0:x0 + w] += 8.0
    m[:, :, ::7, ::11] = float("nan")
  return rows.contiguous(), smooth.contiguous()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--skip_network", action="store_true", help="leave out (d)")
  ap.add_argument("--skip_host", action="store_true", help="leave out (h)")
  opt = ap.parse_args()
  assert torch.cuda.is_available(), "needs a GPU"
  dev = "cuda:0"
  g = torch.Generator(device=dev).manual_seed(1)
  rows = {}
  B, H, W = 4, 375, 1242
  n = B * H * W
  shape = "%dx%dx%d" % (B, H, W)
  by_rows, smooth = scenes(B, H, W, dev, g)
  flt = dfm.DisparityFilter(H, W, batch=B, tol_abs=1.0, max_diff=1.0, max_size=200, device=dev)

  # the composition agrees with the kernel before anything is timed
  for name, m in (("rows", by_rows), ("smooth", smooth)):
    e, ref = flt.edges(m), torch_edge(m, 1.0, 0.0)
    same_jump = (e.jump == ref[2]) | (torch.isnan(e.jump) & torch.isnan(ref[2]))
    print("%s scene: elements where the composition and as_disp_edge_check differ: code %d, valid %d, jump %d, counts %d" % (
        name, int((ref[0] != e.code).sum()), int((ref[1] != e.valid).sum()), int((~same_jump).sum()), int((ref[3] != e.counts).sum())))
    flt(m)
    print("%s scene: share of each code after both stages, image 0: %s" % (name, flt.fractions()[0].round(4).tolist()))
    s = flt.speckles(m)
    print("%s scene: speckle pass alone, image 0: %d components, largest %d pixels" % (
        name, int((s.label[0].flatten() == torch.arange(H * W, device=dev)).sum()), int(s.size[0].max())))

  e = flt.edges(smooth)

  def edge_code_only():
    nat.call("as_disp_edge_check", nat.ptr(smooth), None, B, H, W, 1.0, 0.0, nat.ptr(e.code), None, None, None, nat.stream())
  legs = {"(a) as_disp_edge_check, all outputs": lambda: flt.edges(smooth), "(a) as_disp_edge_check, code only": edge_code_only,
          "(c) torch composition of the edge check": lambda: torch_edge(smooth, 1.0, 0.0)}
  nbytes = {"(a) as_disp_edge_check, all outputs": n * (4 + 1 + 4 + 4) + B * 28, "(a) as_disp_edge_check, code only": n * 5}
  for name, v in alternate(legs, opt.rounds).items():
    rows["%s %s" % (name, shape)] = summary(v, nbytes.get(name))

  one = torch.full((B, 1, H, W), 12.5, device=dev)
  yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
  board = torch.where(((yy + xx) % 2 == 0).view(1, 1, H, W), one, torch.full((), float("nan"), device=dev)).contiguous()
  legs = {"(b) as_disp_speckle, scene of per-row levels": lambda: flt.speckles(by_rows),
          "(b) as_disp_speckle, smooth scene": lambda: flt.speckles(smooth),
          "(b) DisparityFilter (both stages), smooth scene": lambda: flt(smooth),
          "(x) as_disp_speckle, one component": lambda: flt.speckles(one),
          "(x) as_disp_speckle, checkerboard": lambda: flt.speckles(board)}
  speckle_bytes = n * (4 + 4 + 4 + 1 + 4) + B * 28                 # disp in; label, size, code, valid out, each once
  for name, v in alternate(legs, opt.rounds).items():
    rows["%s %s" % (name, shape)] = summary(v, None if "both stages" in name else speckle_bytes)

  if not opt.skip_host:
    import numpy as np
    from scipy import ndimage
    size_back = torch.empty(B, 1, H, W, dtype=torch.int32, device=dev)

    def host_route(m):
      host = m.cpu().numpy()                                # synchronises
      us = (host >= 0) & ~np.isposinf(host)
      out = np.zeros(host.shape, dtype=np.int32)
      for b in range(B):
        lab, _ = ndimage.label(us[b, 0])
        out[b, 0] = np.where(us[b, 0], np.bincount(lab.reshape(-1))[lab], 0)
      size_back.copy_(torch.from_numpy(out))
    host_route(smooth)
    s = dfm.DisparityFilter(H, W, batch=B, max_diff=float("inf"), device=dev).speckles(smooth)
    print("host route against as_disp_speckle at max_diff = +inf: sizes differ in %d pixels" % int((size_back != s.size).sum()))
    inf_flt = dfm.DisparityFilter(H, W, batch=B, max_diff=float("inf"), device=dev)
    legs = {"(h) copy out, scipy.ndimage.label + bincount, copy back": lambda: host_route(smooth),
            "(h) as_disp_speckle at max_diff = +inf, synchronised": lambda: inf_flt.speckles(smooth)}
    for name, v in alternate(legs, min(opt.rounds, 3), clock=wall).items():
      rows["%s %s (wall clock)" % (name, shape)] = summary(v)

  if not opt.skip_network:
    from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
    from adaptive_stereo.utils import synthetic as syn
    k = 4
    fnet, snet = FeatureExtractorNetwork(k), StereoNet(k, 1, 0, maxdisp=192)
    fnet.load_state_dict(syn.synthetic_state_dict(fnet.state_dict(), seed=123))
    snet.load_state_dict(syn.synthetic_state_dict(snet.state_dict(), seed=123, logit_gain=20.0))
    fnet, snet = fnet.to(dev).eval(), snet.to(dev).eval()
    left, right = (t.to(dev).contiguous() for t in syn.stereo_pair(B, H, W, seed=1))
    plain = cons.BothViewInference(fnet, snet, H, W, batch=B).capture(left, right)
    filtered = dfm.FilteredBothViewInference(fnet, snet, H, W, batch=B).capture(left, right)
    a, b = plain(left, right), filtered(left, right)
    print("filtered against plain replay: disp_l equal %s, disp_r equal %s, code_l equal %s" % (
        torch.equal(a[0], b[0]), torch.equal(a[1], b[1]), torch.equal(a[2].code_l, b[2].code_l)))
    print("share of each code of the network's left view after check and filter, image 0:",
          filtered.filter.fractions()[0].round(4).tolist())
    legs = {"(d) BothViewInference, replayed": lambda: plain(left, right),
            "(d) FilteredBothViewInference, replayed": lambda: filtered(left, right)}
    for name, v in alternate(legs, opt.rounds).items():
      rows["%s %s k=%d" % (name, shape, k)] = summary(v)

  rows["what"] = ("device events around 200 back-to-back calls after 10 warm-up calls; %d rounds, the legs of a group alternating; "
                  "bytes are algorithmic (each tensor once); the (h) legs are wall clock around synchronised calls" % opt.rounds)
  for name, r in rows.items():
    print(name, json.dumps(r))
  if opt.out:
    with open(opt.out, "w") as f:
      json.dump(rows, f, indent=1, sort_keys=True)
      f.write("\n")


if __name__ == "__main__":
  sys.exit(main())
