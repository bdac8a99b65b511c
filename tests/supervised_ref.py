"""The supervised training step (reference train.py:204-223) composed from the oracle's functions (oracle/stereo_oracle.py), and
a host restatement of the two-scale loss's per-pixel arithmetic for the kernel tests of csrc/supervised.hip.

``supervised_step`` is the loop body of the reference's train(): both feature extractions in train mode, StereoNet.forward,
khamis_robust_loss_multiscale(scales=[s, s + k]) — the equal-weight sum, refined scale first —, backward, optional
clip_grad_norm_ on stereo_net, Adam over (stereo_net, feature_net).  tests/test_supervised_ref_cpu.py holds it to
tests/golden/supervised_step.npz, which the reference's own modules produced (tests/golden/make_golden_supervised.py).

Per pixel (utils/loss_functions.py:15), with d = gt - pred where gt > 0:
  value = sqrt(d^2 + 4) / 2 - 1            every operation rounded to float32, as the reference's element-wise chain
  slope = d value / d pred = -d / (2 sqrt(d^2 + 4))
"""
import numpy as np
import torch

from oracle import stereo_oracle as orc

F32 = np.float32


def supervised_step(feat_p, stereo_p, opt_state, left, right, gt, k, input_scale=0, maxdisp=192, lr=1e-5, clip=False):
  """feat_p / stereo_p: orc.make_params(..., True) dictionaries, updated in place (gradients stay in ``.grad``).
  -> {"total_loss", "khamis_robust_loss/{s}", "khamis_robust_loss/{s+k}", "outputs"}"""
  for p in list(feat_p.values()) + list(stereo_p.values()):
    p.grad = None
  fl = orc.feature_extractor(feat_p, left, k, True)
  fr = orc.feature_extractor(feat_p, right, k, True)
  out = orc.stereo_forward(stereo_p, left, fl, fr, k, input_scale, maxdisp, "l", True, False)
  res = {"total_loss": 0}
  for scale in (input_scale, input_scale + k):
    this = orc.khamis_robust_loss(out["pred_disp_l/%d" % scale], gt)
    res["khamis_robust_loss/%d" % scale] = this
    res["total_loss"] = res["total_loss"] + this
  res["total_loss"].backward()
  if clip:
    orc.clip_grad_norm([p.grad for p in stereo_p.values() if p.requires_grad])
  with torch.no_grad():
    for name, group in (("stereo", stereo_p), ("feature", feat_p)):       # train.py:165
      for kk, p in group.items():
        if p.requires_grad and p.grad is not None:
          orc.adam_step(p, p.grad, opt_state.setdefault((name, kk), {}), lr)
  res = {name: (v.detach() if torch.is_tensor(v) else v) for name, v in res.items()}
  res["outputs"] = out
  return res


def zero_gradient_names(feat_keys, stereo_keys):
  """("feature." / "stereo." + name) of the parameters whose gradient is analytically zero in a train-mode step: every
  convolution bias in front of a train-mode BatchNorm (the batch mean removes it), conv3d_alone.bias (a constant added to every
  logit of a pixel: soft-max does not see it) and the feature extractor's conv_alone.bias (the cost volume is a difference of
  the two feature maps).  What autograd returns for them is rounding noise."""
  out = set()
  for prefix, keys in (("feature.", feat_keys), ("stereo.", stereo_keys)):
    keys = set(keys)
    for key in keys:
      if ".conv2." in key:
        continue                                        # BasicBlock.conv2 is never run: no gradient at all
      if key.endswith(".0.bias") and (key[:-len("0.bias")] + "1.running_mean") in keys:
        out.add(prefix + key)
  out.add("stereo.conv3d_alone.bias")
  out.add("feature.conv_alone.bias")
  return out


# ---- the kernels' per-pixel arithmetic on the host ---------------------------------------------------------------------------
def valid(gt):
  """gt > 0; NaN is not valid"""
  with np.errstate(invalid="ignore"):
    return np.asarray(gt, dtype=F32) > 0


def pixel_values(pred, gt):
  """float32 [n]: sqrt(d * d + 4) / 2 - 1 with every operation rounded to float32, 0 where gt is not valid"""
  pred, gt = np.asarray(pred, dtype=F32).reshape(-1), np.asarray(gt, dtype=F32).reshape(-1)
  m = valid(gt)
  d = np.where(m, gt, F32(0)) - np.where(m, pred, F32(0))
  d = d.astype(F32)
  v = (np.sqrt((d * d).astype(F32) + F32(4)).astype(F32) / F32(2)).astype(F32) - F32(1)
  return np.where(m, v.astype(F32), F32(0)).astype(F32)


def loss_from_values(values, gt):
  """(float64 sum of the float32 per-pixel values) / max(count, 1) in float64, and the count"""
  n = max(int(valid(gt).sum()), 1)
  return float(values.astype(np.float64).sum()) / n, n


def pixel_slopes64(pred, gt):
  """float64: -d / (2 sqrt(d^2 + 4)) from the float32 inputs, 0 where gt is not valid; same shape as pred"""
  p, g = np.asarray(pred, dtype=F32).astype(np.float64), np.asarray(gt, dtype=F32)
  m = valid(g)
  d = np.where(m, g.astype(np.float64), 0.0) - np.where(m, p, 0.0)
  return np.where(m, -d / (2.0 * np.sqrt(d * d + 4.0)), 0.0)


# ---- inputs shared by the tests and tests/tools/reassociation_bound_supervised.py ------------------------------------------------
def ground_truth(pred_eval, seed):
  """The tests' synthetic ground truth: an eval-mode refined prediction + U(-3, 3), zero (not valid) at [:, :, ::3, ::5]"""
  noise = torch.rand(pred_eval.shape, generator=torch.Generator().manual_seed(seed)) * 6.0 - 3.0
  gt = (pred_eval.detach().cpu() + noise).contiguous()
  gt[:, :, ::3, ::5] = 0.0
  return gt
