"""tests/tools/reassociation_bound.py's question for the SUPERVISED step: how far do the reference's own losses and gradients
move when nothing but the fp32 summation order of its convolutions changes?

Same method: the supervised step composed from the oracle (tests/supervised_ref.py, held to the reference's own run by
tests/test_supervised_ref_cpu.py) is run as it is and with every convolution summed tap by tap (reassociation_bound.TapSum,
3-D only and all convolutions, both tap orders), from the same state, without moving the parameters.  Cases: the shape and
the three pairs of tests/test_gpu_supervised.py's three-step test, and the two cases of tests/golden/supervised_step.npz.
Written to tests/golden/reassociation_bound_supervised.json per case and variant:

  loss_delta                      |delta| of each of the three losses (largest)
  worst_tensor_rel_l2             max over parameter tensors of |g' - g|_2 / |g|_2, every tensor except the 19 whose gradient is
                                  analytically zero (supervised_ref.zero_gradient_names); worst_zero_abs_over_weight is the
                                  largest |g| among those 19, relative to max |g| of their layer's weight gradient
  whole_{stereo,feature}_rel_l2   the same over each network's whole gradient vector

tests/test_gpu_supervised.py takes 2 x the worst row of its gain class (the project's rule: a GPU kernel is one more
reassociation on top of the reference's own; tests/test_gpu_end_to_end.py:33-40), tests/test_supervised_ref_cpu.py 1 x.

Run in the build container (CPU):  python tests/tools/reassociation_bound_supervised.py
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import conftest                                          # noqa: E402,F401
from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork   # noqa: E402
from adaptive_stereo.utils import synthetic as syn       # noqa: E402
from oracle import stereo_oracle as orc                  # noqa: E402
import supervised_ref as sref                            # noqa: E402
from reassociation_bound import TapSum                   # noqa: E402

CASES = {
  "three_steps_64x160_pair41": dict(B=2, H=64, W=160, k=3, s=0, maxdisp=64, gain=5.0, pair_seed=41),
  "three_steps_64x160_pair42": dict(B=2, H=64, W=160, k=3, s=0, maxdisp=64, gain=5.0, pair_seed=42),
  "three_steps_64x160_pair43": dict(B=2, H=64, W=160, k=3, s=0, maxdisp=64, gain=5.0, pair_seed=43),
  "fixture_75x131": dict(B=1, H=75, W=131, k=3, s=0, maxdisp=96, gain=20.0, pair_seed=41),
}
GT_SEED = 97


def states(meta):
  fnet = FeatureExtractorNetwork(meta["k"])
  snet = StereoNet(meta["k"], 1, meta["s"], maxdisp=meta["maxdisp"])
  return (syn.synthetic_state_dict(fnet.state_dict(), seed=123),
          syn.synthetic_state_dict(snet.state_dict(), seed=123, logit_gain=meta["gain"]))


def run(meta, left, right, gt, shim):
  fsd, ssd = states(meta)
  fp, sp = orc.make_params(fsd, True), orc.make_params(ssd, True)
  saved = orc.F
  orc.F = shim if shim is not None else saved
  try:
    res = sref.supervised_step(fp, sp, {}, left, right, gt, meta["k"], meta["s"], meta["maxdisp"], lr=0.0)
  finally:
    orc.F = saved
  grads = {}
  for net, group in (("stereo", sp), ("feature", fp)):
    for name, p in group.items():
      if p.requires_grad and p.grad is not None:
        grads["%s.%s" % (net, name)] = p.grad.detach().clone()
  losses = [float(v) for name, v in res.items() if name != "outputs"]
  return losses, grads, sref.zero_gradient_names(fsd.keys(), ssd.keys())


def grad_rows(base, other, zero_names):
  worst, zero = (0.0, ""), 0.0
  whole = {"stereo": [0.0, 0.0], "feature": [0.0, 0.0]}
  for name, g in base.items():
    diff = other[name].double() - g.double()
    net = name.split(".", 1)[0]
    whole[net][0] += float(diff.pow(2).sum()); whole[net][1] += float(g.double().pow(2).sum())
    if name in zero_names:
      wmax = float(base[name[:-len("bias")] + "weight"].abs().max())
      zero = max(zero, float(g.abs().max()) / wmax, float(other[name].abs().max()) / wmax)
      continue
    worst = max(worst, (float(diff.norm() / g.double().norm()), name))
  return {"worst_tensor_rel_l2": worst[0], "worst_tensor": worst[1], "worst_zero_abs_over_weight": zero,
          "whole_stereo_rel_l2": (whole["stereo"][0] / whole["stereo"][1]) ** 0.5,
          "whole_feature_rel_l2": (whole["feature"][0] / whole["feature"][1]) ** 0.5}


def main():
  torch.set_num_threads(8)
  report = {"torch": torch.__version__, "what": __doc__.split("\n")[0], "cases": {}}
  for case, meta in CASES.items():
    left, right = syn.stereo_pair(meta["B"], meta["H"], meta["W"], seed=meta["pair_seed"], disparities=(4.0, 7.0))
    fsd, ssd = states(meta)
    pred = orc.forward_only(fsd, ssd, left, right, meta["k"], meta["s"], meta["maxdisp"])[0]["pred_disp_l/%d" % meta["s"]]
    gt = sref.ground_truth(pred, GT_SEED)
    base_losses, base_grads, zero_names = run(meta, left, right, gt, None)
    rows = {}
    for label, shim in (("conv3d_taps_fwd", TapSum(+1, (3,))), ("conv3d_taps_rev", TapSum(-1, (3,))),
                        ("all_convs_taps_fwd", TapSum(+1, (2, 3))), ("all_convs_taps_rev", TapSum(-1, (2, 3)))):
      losses, grads, _ = run(meta, left, right, gt, shim)
      rows[label] = dict(grad_rows(base_grads, grads, zero_names),
                         loss_delta=max(abs(a - b) for a, b in zip(losses, base_losses)), total_loss=base_losses[0])
      print(case, label, rows[label], flush=True)
    report["cases"][case] = {"gain": meta["gain"], "rows": rows}
  with open(os.path.join(HERE, "..", "golden", "reassociation_bound_supervised.json"), "w") as f:
    json.dump(report, f, indent=1, sort_keys=True)


if __name__ == "__main__":
  main()
