"""Times the adaptation step of the validated modes (adaptive_stereo/control.py) with HIP events at KITTI size: one pair of
375 x 1242 per step, k = 4, maxdisp 192.  Five steps, alternating in one process after warm-up:

  captured NONSTOP          OnlineAdapter.step replaying its hipGraph (the benchmark's step)
  eager VS+ER               AdaptationLoop.process, IN_PROGRESS, host-side gate (one read-back per step, ~2 x 130 launches)
  gated VS, no insertion    AdaptationLoop(captured=True), mode VS, threshold -inf: gate + refused store + gated clip/Adam
  gated VS, every insertion the same with threshold +inf, a fresh batch index per step and the step's uniform number pinned to 0
                            (r = 1: a full buffer replaces slot 0 every time): the store kernel runs, the update is withheld
  gated VS+ER               mode VS+ER, no insertion: the replay pair's forward and backward in the same graph

Per variant: milliseconds per step by HIP events (median [min .. max] of the rounds) and the host's wall time per call of
step() / process() (what the issuing thread spends; the eager loop's includes its read-back).  Then the store kernel alone at one
and four pairs against the bytes it moves.  There is no pass/fail time.

usage (GPU box): python tests/tools/time_gated_step.py [--out profiles/gated_step_timing.txt]
"""
import argparse
import math
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "adaptive-stereo-icra-2021_amd"))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import numpy as np
import torch

from adaptive_stereo import _native as nat
from adaptive_stereo import control
from adaptive_stereo.adaptation import OnlineAdapter
from adaptive_stereo.control import AdaptationLoop, State
from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
from adaptive_stereo.utils import synthetic as syn

DEV = "cuda:0"
H, W, K, MAXDISP = 375, 1242, 4, 192
ROUNDS, ROUND_SECONDS = 5, 0.4
NEVER = 1 << 30            # ovs_validate_hz: no validation inside the timed rounds


def nets():
  fnet, snet = FeatureExtractorNetwork(K), StereoNet(K, 1, 0, maxdisp=MAXDISP)
  fnet.load_state_dict(syn.synthetic_state_dict(fnet.state_dict(), seed=123), strict=True)
  snet.load_state_dict(syn.synthetic_state_dict(snet.state_dict(), seed=123, logit_gain=20.0), strict=True)
  return fnet.to(DEV), snet.to(DEV)


def events(fn, calls):
  """-> (device ms per call, host wall ms per call)."""
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  e0.record()
  t0 = time.perf_counter()
  for _ in range(calls):
    fn()
  host = (time.perf_counter() - t0) * 1e3 / calls
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / calls, host


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(HERE, "..", "..", "profiles", "gated_step_timing.txt"))
  args = ap.parse_args()
  lines = []

  def say(text=""):
    print(text, flush=True)
    lines.append(text)

  left, right = (t.to(DEV) for t in syn.stereo_pair(1, H, W, seed=41))
  rl, rr = (t.to(DEV) for t in syn.stereo_pair(1, H, W, seed=42))
  rgt = (torch.rand(1, 1, H, W, generator=torch.Generator().manual_seed(97)) * 60 + 1).to(DEV)
  replay = (rl, rr, rgt)

  nonstop = OnlineAdapter(*nets(), H, W)
  nonstop.capture(left, right)
  nl, nr = nonstop.graph_inputs()

  def loop(mode, captured, threshold):
    return AdaptationLoop(OnlineAdapter(*nets(), H, W), mode=mode, ovs_buffer_size=10, ovs_validate_hz=NEVER,
                          ood_threshold=threshold, captured=captured)
  eager = loop("VS+ER", False, float("-inf"))
  quiet = loop("VS", True, float("-inf"))
  insert = loop("VS", True, float("inf"))
  gated_er = loop("VS+ER", True, float("-inf"))
  counter = [0]

  class PinnedUniform(object):            # the captured loops' random.random(): only "insert" ever uses the number
    random = staticmethod(lambda: 0.0)
  control.random = PinnedUniform

  def fresh_index():
    counter[0] += 1
    return counter[0]
  variants = [("captured NONSTOP", lambda: nonstop.step(nl, nr)),
              ("eager VS+ER", lambda: eager.process(left, right, 0, replay=replay)),
              ("gated VS, no insertion", lambda: quiet.process(left, right, 0)),
              ("gated VS, every insertion", lambda: insert.process(left, right, fresh_index())),
              ("gated VS+ER", lambda: gated_er.process(left, right, 0, replay=replay))]
  calls = []
  for name, fn in variants:
    for _ in range(3):
      fn()
    torch.cuda.synchronize()
    calls.append(max(5, int(math.ceil(ROUND_SECONDS * 1e3 / events(fn, 5)[0]))))
  for lp in (quiet, insert, gated_er):
    assert lp.graph_count() == 1 and lp.state_machine.state() == State.IN_PROGRESS
  dev_ms, host_ms = [[] for _ in variants], [[] for _ in variants]
  for _ in range(ROUNDS):
    for i, (name, fn) in enumerate(variants):
      d, h = events(fn, calls[i])
      dev_ms[i].append(d); host_ms[i].append(h)
  for lp in (quiet, insert, gated_er):
    lp.sync()
  say("adaptation step, one pair of %dx%d, k=%d, maxdisp %d; device %s, torch %s" % (H, W, K, MAXDISP,
      torch.cuda.get_device_name(0), torch.__version__))
  say("per step: device ms by HIP events, median [min .. max] of %d alternating rounds | host wall ms per call, median" % ROUNDS)
  for (name, _), d, h, c in zip(variants, dev_ms, host_ms, calls):
    say("  %-26s %8.3f [%8.3f .. %8.3f] | host %7.3f   %d steps per round" % (name, float(np.median(d)), min(d), max(d),
        float(np.median(h)), c))
  med = [float(np.median(d)) for d in dev_ms]
  say("  eager VS+ER / gated VS+ER: %.2fx" % (med[1] / med[4]))
  say("  gated VS (no insertion) - captured NONSTOP: %+.1f us; with insertion (store runs, backward still runs, update withheld): "
      "%+.1f us" % ((med[2] - med[0]) * 1e3, (med[3] - med[0]) * 1e3))
  say("  counters: quiet updates %d; insert adds %d of offers %d, updates %d" % (quiet.gradient_updates,
      insert.state_machine.ovs.counters()[2], insert.state_machine.ovs.counters()[1], insert.gradient_updates))

  # the store kernel alone: 2 * n floats read and 2 * n written per call
  say("as_reservoir_store alone (slot 0 of 4), HIP events over 200 launches:")
  slot = torch.zeros(1, dtype=torch.int32, device=DEV)
  for pairs in (1, 4):
    n = pairs * 3 * H * W
    src = torch.rand(2, n, device=DEV)
    buf = torch.zeros(2, 4, n, device=DEV)
    fn = lambda: nat.call("as_reservoir_store", nat.ptr(src[0]), nat.ptr(src[1]), n, nat.ptr(slot), 4, nat.ptr(buf[0]),
                          nat.ptr(buf[1]), nat.stream())
    for _ in range(10):
      fn()
    t = [events(fn, 200)[0] for _ in range(ROUNDS)]
    moved = 4.0 * n * 4
    say("  %d pair(s): %7.2f us [%7.2f .. %7.2f], %.1f MB moved, %.0f GB/s" % (pairs, float(np.median(t)) * 1e3, min(t) * 1e3,
        max(t) * 1e3, moved / 1e6, moved / (float(np.median(t)) * 1e-3) / 1e9))
  with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
