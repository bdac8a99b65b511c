"""Times the supervised training step (adaptive_stereo/training.py) with HIP events at the shape of the reference's 16X training
scripts (experiments/training/*_16X.sh): batch 8 of 320 x 960, k = 4, maxdisp 192.  Four steps, alternating in one process
after warm-up, each over at least 2 s in all:

  captured, fused loss     SupervisedTrainer.step replaying its hipGraph (the two-scale loss one node: csrc/supervised.hip)
  captured, composed loss  the same step with khamis_robust_loss_multiscale + autograd (two as_khamis_fwd, two as_khamis_bwd,
                           as_upsample_bilinear_bwd and autograd's additions) in its place, captured the same way
  eager, fused loss        SupervisedTrainer._step_eager
  captured adaptation      OnlineAdapter.step at the same shape, for scale

Milliseconds per step: median [min .. max] of the rounds.  There is no pass/fail time.

usage (GPU box): python tests/tools/time_train_step.py [--out profiles/train_step_timing.txt]
"""
import argparse
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "adaptive-stereo-icra-2021_amd"))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import numpy as np
import torch

from adaptive_stereo.adaptation import OnlineAdapter
from adaptive_stereo.training import SupervisedTrainer
from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
from adaptive_stereo.utils import synthetic as syn
from adaptive_stereo.utils.loss_functions import khamis_robust_loss_multiscale

DEV = "cuda:0"
B, H, W, K, MAXDISP = 8, 320, 960, 4, 192
ROUNDS, ROUND_SECONDS = 5, 0.5


class ComposedTrainer(SupervisedTrainer):
  def _losses(self, gt, out):
    return khamis_robust_loss_multiscale({"gt_disp_l/0": gt}, out, scales=[self.scale, self.coarse_scale], gt_disp_scale=self.scale)


def nets():
  fnet, snet = FeatureExtractorNetwork(K), StereoNet(K, 1, 0, maxdisp=MAXDISP)
  fnet.load_state_dict(syn.synthetic_state_dict(fnet.state_dict(), seed=123), strict=True)
  snet.load_state_dict(syn.synthetic_state_dict(snet.state_dict(), seed=123, logit_gain=20.0), strict=True)
  return fnet.to(DEV), snet.to(DEV)


def events(fn, calls):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(calls):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / calls


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(HERE, "..", "..", "profiles", "train_step_timing.txt"))
  args = ap.parse_args()
  lines = []

  def say(text=""):
    print(text, flush=True)
    lines.append(text)

  left, right = (t.to(DEV) for t in syn.stereo_pair(B, H, W, seed=41))
  fused, composed, eager = SupervisedTrainer(*nets()), ComposedTrainer(*nets()), SupervisedTrainer(*nets())
  fused.feature_net.eval(); fused.stereo_net.eval()
  with torch.no_grad():
    pred = fused.stereo_net(left, fused.feature_net(left), fused.feature_net(right), "l")["pred_disp_l/0"]
  gt = pred + (torch.rand(pred.shape, generator=torch.Generator().manual_seed(97)) * 6.0 - 3.0).to(DEV)
  gt[:, :, ::3, ::5] = 0.0
  # agreement first: the two losses are the same number to an ulp, and so is the first step's result
  a, b = fused.step(left, right, gt), composed.step(left, right, gt)
  torch.cuda.synchronize()
  say("first step: total loss fused %.7f, composed %.7f" % (float(a["total_loss"]), float(b["total_loss"])))
  assert abs(float(a["total_loss"]) - float(b["total_loss"])) <= 4e-7 * abs(float(b["total_loss"]))
  eager.step(left, right, gt)
  fused.capture(left, right, gt); composed.capture(left, right, gt)
  adapter = OnlineAdapter(*nets(), H, W)
  adapter.capture(left, right)
  fl, fr, fg = fused.graph_inputs()
  cl, cr, cg = composed.graph_inputs()
  al, ar = adapter.graph_inputs()
  variants = [("captured, fused loss", lambda: fused.step(fl, fr, fg)),
              ("captured, composed loss", lambda: composed.step(cl, cr, cg)),
              ("eager, fused loss", lambda: eager._step_eager(left, right, gt)),
              ("captured adaptation step", lambda: adapter.step(al, ar))]
  calls = []
  for name, fn in variants:
    for _ in range(3):
      fn()
    torch.cuda.synchronize()
    calls.append(max(5, int(math.ceil(ROUND_SECONDS * 1e3 / events(fn, 5)))))
  times = [[] for _ in variants]
  for _ in range(ROUNDS):
    for i, (name, fn) in enumerate(variants):
      times[i].append(events(fn, calls[i]))
  say("supervised training step, batch %d of %dx%d, k=%d, maxdisp %d; device %s, torch %s" % (B, H, W, K, MAXDISP,
      torch.cuda.get_device_name(0), torch.__version__))
  say("milliseconds per step: median [min .. max] of %d alternating rounds, HIP events" % ROUNDS)
  for (name, _), t, c in zip(variants, times, calls):
    say("  %-26s %8.3f [%8.3f .. %8.3f]   %d steps per round, %.1f s in all" % (name, float(np.median(t)), min(t), max(t), c,
        sum(t) * c / 1e3))
  diff = [c_ - f_ for f_, c_ in zip(times[0], times[1])]
  say("  composed - fused, round by round (us): " + ", ".join("%.1f" % (d * 1e3) for d in diff))
  with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
