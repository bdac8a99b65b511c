"""Holds tests/supervised_ref.py — the supervised training step composed from the oracle's functions — to
tests/golden/supervised_step.npz, which the reference's own modules produced (tests/golden/make_golden_supervised.py): three
steps of the training loop's body on one pair with the learning rate halved before the third, then a step whose ground truth
has no valid pixel.  As in the fixture's run, weights and BatchNorm buffers are drawn anew before every step but the first
(seed 123 + step) while Adam's moments and step count carry over: every step starts from a state both sides share exactly
(two fp32 implementations of this network do not stay together over consecutive steps: make_golden_supervised.py says why),
and what the optimizer carries is in every comparison.  CPU only.

Tolerances are those tests/test_oracle_golden.py applies to the same kinds of quantity: losses 2e-6 absolute (+ 1e-6 relative:
the supervised losses are 5 .. 20, the adaptation loss it was set for is below 1), gradients 1e-6 x gain + 2e-4 x max|g|
absolute and 2e-3 relative per element, weights after a step after_step_atol's 2e-6 (+ 2.1 lr where the reference's own
gradient is rounding noise) and 1e-5 relative, BatchNorm buffers 2e-6 / 1e-5.  Every gradient tensor is also compared in
relative L2 against the element-wise tolerance's relative part, 2e-3: 61 tensors, worst seen 4.4e-6 (64x160) and 4.2e-6
(75x131).  The 19 tensors whose gradient is analytically zero (supervised_ref.zero_gradient_names) hold rounding noise in both
implementations and are held to an absolute bound alone: the absolute allowance of an element of the same layer's weight
gradient, 1e-6 x gain + 2e-4 x max|g_weight| (the bias gradient is the plain sum of the terms the weight gradient sums with
activations of order 1 as factors).  The test asserts that the biases the reference's own gradients put below 1e-4 of their
layer's weight gradient are exactly those 19 (fixture: noise up to 4.7e-6 of it, the smallest true bias gradient 0.11).
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, parity_note
from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
from adaptive_stereo.utils import synthetic as syn
from oracle import stereo_oracle as orc
import supervised_ref as sref

SUB_LIMIT = 256       # must match tests/golden/make_golden_supervised.py
CASES = ["64x160", "75x131"]


class SupervisedGolden(object):
  def __init__(self):
    self.z = np.load(os.path.join(GOLDEN_DIR, "supervised_step.npz"), allow_pickle=False)

  def meta(self, case):
    return json.loads(str(self.z[case + "/meta"]))

  def no_grad_keys(self, case):
    return json.loads(str(self.z[case + "/no_grad_keys"]))

  def gt(self, case):
    return torch.from_numpy(self.z[case + "/gt"])

  def scalar(self, case, step, name):
    return float(self.z["%s/step%d/%s" % (case, step, name)])

  def counters(self, case, step):
    return json.loads(str(self.z["%s/step%d/counters" % (case, step)]))

  def pack(self, case, step, kind):
    """name -> (stored values, shape): whole tensors up to SUB_LIMIT values, else syn.subsample(t, SUB_LIMIT)"""
    key = "%s/step%d/%s" % (case, step, kind)
    flat, out, at = torch.from_numpy(self.z[key]), {}, 0
    for name, shape, n in json.loads(str(self.z[key + "__index"])):
      out[name] = (flat[at:at + n], tuple(shape))
      at += n
    assert at == flat.numel()
    return out


def stored(t):
  t = t.detach().float()
  return t.reshape(-1) if t.numel() <= SUB_LIMIT else syn.subsample(t, SUB_LIMIT)


@pytest.fixture(scope="module")
def gold():
  return SupervisedGolden()


def build_states(meta, seed=123):
  fnet = FeatureExtractorNetwork(meta["k"])
  snet = StereoNet(meta["k"], 1, meta["s"], maxdisp=meta["maxdisp"])
  return (syn.synthetic_state_dict(fnet.state_dict(), seed=seed),
          syn.synthetic_state_dict(snet.state_dict(), seed=seed, logit_gain=meta["gain"]))


def close(got, exp, atol, rtol, what):
  err = (got.double() - exp.double()).abs()
  tol = atol + rtol * exp.double().abs()
  assert bool((err <= tol).all()), "%s: max abs err %.3e, %d/%d over" % (what, float(err.max()), int((err > tol).sum()), err.numel())


@pytest.mark.parametrize("case", CASES)
def test_composed_supervised_step_matches_the_reference(case, gold):
  meta = gold.meta(case)
  torch.set_num_threads(8)
  k, s, scale = meta["k"], meta["s"], max(1.0, meta["gain"])
  left, right = syn.stereo_pair(meta["B"], meta["H"], meta["W"], seed=meta["pair_seed"], disparities=tuple(meta["disparities"]))
  for name, t in (("left", left), ("right", right)):
    sm, ss = syn.checksum(t)
    es, ess = gold.z["%s/sum__%s" % (case, name)]
    assert abs(sm - es) <= 1e-6 * abs(es) and abs(ss - ess) <= 1e-6 * abs(ess), "the synthetic pair differs from the fixture's"
  gt = gold.gt(case)
  assert abs(float((gt > 0).float().mean()) - 0.93) < 0.01
  fsd, ssd = build_states(meta)
  fp, sp = orc.make_params(fsd, True), orc.make_params(ssd, True)
  groups = {"stereo": sp, "feature": fp}
  zero_names = sref.zero_gradient_names(fsd.keys(), ssd.keys())
  assert len(zero_names) == 19
  dead = set(gold.no_grad_keys(case))
  opt_state, was_noise = {}, {}
  worst, worst0 = (0.0, ""), 0.0
  for step in range(meta["steps"] + 1):
    lr = meta["lrs"][step]
    this_gt = gt if step < meta["steps"] else torch.zeros_like(gt)
    if step > 0:
      with torch.no_grad():            # as the fixture's run: weights and buffers drawn anew, in place; Adam's state stays
        for group, sd in zip((fp, sp), build_states(meta, meta["weight_seed"] + step)):
          for name, p in group.items():
            p.copy_(sd[name])
    res = sref.supervised_step(fp, sp, opt_state, left, right, this_gt, k, s, meta["maxdisp"], lr=lr)
    for name in ("total_loss", "khamis_robust_loss/%d" % s, "khamis_robust_loss/%d" % (s + k)):
      ref = gold.scalar(case, step, name)
      tol = 2e-6 + 1e-6 * abs(ref)
      assert abs(float(res[name]) - ref) <= tol, (step, name, float(res[name]), ref)
    if step == meta["steps"]:
      assert float(res["total_loss"]) == 0.0
    ref_grads = gold.pack(case, step, "grad") if step < meta["steps"] else {}
    compared, noise = 0, set()
    for net in ("stereo", "feature"):
      for name, p in groups[net].items():
        full = "%s.%s" % (net, name)
        if not p.requires_grad:
          continue
        if full in dead:
          assert p.grad is None and orc.conv2_is_dead(name)
          continue
        if step == meta["steps"]:
          assert float(p.grad.abs().max()) == 0.0, full          # no valid pixel: exact zeros
          continue
        exp, shape = ref_grads[full]
        assert tuple(p.grad.shape) == shape
        got = stored(p.grad)
        gmax = float(p.grad.abs().max())
        if full.endswith(".bias"):
          # a bias gradient is the plain sum of the terms its layer's weight gradient sums with activations of order 1 as
          # factors: where it is analytically zero, what is left is the rounding of that sum, and it is measured against
          # the weight gradient's size (fixture: at most 4.7e-6 of it; the smallest true bias gradient is 0.11 of it)
          wmax = float(ref_grads[full[:-len("bias")] + "weight"][0].abs().max())
          if float(exp.abs().max()) <= 1e-4 * wmax:
            noise.add(full)
            # the absolute allowance an element of that weight gradient has
            close(got, exp, 1e-6 * scale + 2e-4 * wmax, 0.0, "step %d grad %s (analytically zero)" % (step, full))
            continue
        close(got, exp, 1e-6 * scale + 2e-4 * gmax, 2e-3, "step %d grad %s" % (step, full))
        rel = float((got.double() - exp.double()).norm() / exp.double().norm())
        worst = max(worst, (rel, "step %d %s" % (step, full)))
        if step == 0:
          worst0 = max(worst0, rel)
        assert rel <= 2e-3, (step, full, rel)          # (the relative part of the element-wise tolerance)
        compared += 1
    if step < meta["steps"]:
      assert noise == zero_names, sorted(noise ^ zero_names)
      assert compared == 61
    # state after the step
    ref_after, counters = gold.pack(case, step, "after"), gold.counters(case, step)
    for net in ("stereo", "feature"):
      for name, p in groups[net].items():
        full = "%s.%s" % (net, name)
        if name.endswith("num_batches_tracked"):
          assert int(p) == counters[full], full
          continue
        exp, shape = ref_after[full]
        assert tuple(p.shape) == shape
        # test_oracle_golden.after_step_atol: 2e-6, and 2.1 lr where the gradient is rounding noise — an Adam step is at
        # most 1.004 lr in size whatever the noise is (Cauchy-Schwarz on m / sqrt(v) with the bias corrections, steps 1 .. 4)
        atol = 2e-6
        if full in zero_names:
          atol = atol + 2.1 * lr
        elif full in ref_grads:
          g = ref_grads[full][0].abs().double()
          was_noise[full] = was_noise.get(full, 0) | (g < 1e-6 * scale)      # (noise in every moment so far)
          atol = atol + 2.1 * lr * was_noise[full].double()
        close(stored(p), exp, atol, 1e-5, "step %d after %s" % (step, full))
  parity_note("supervised_ref[%s]" % case, worst_tensor_rel_l2=worst[0], worst_tensor=worst[1], worst_first_step=worst0)


def test_per_pixel_restatement_equals_the_oracle_loss():
  """supervised_ref.pixel_values / loss_from_values / pixel_slopes64 (what the kernel tests compare with) against the oracle's
  khamis_robust_loss and its autograd on the CPU: loss to float32 rounding of a sum (1e-6 relative), derivative to 3e-7."""
  g = torch.Generator().manual_seed(5)
  pred = (torch.rand(2, 1, 37, 53, generator=g) * 40).requires_grad_(True)
  gt = pred.detach() + torch.rand(2, 1, 37, 53, generator=g) * 12 - 6
  gt[:, :, ::3, ::5] = 0.0
  gt[0, 0, 1, 1] = float("nan"); gt[1, 0, 2, 2] = -3.0
  ref = orc.khamis_robust_loss(pred, torch.nan_to_num(gt, nan=0.0))
  ref.backward()
  v = sref.pixel_values(pred.detach().numpy(), gt.numpy())
  loss, n = sref.loss_from_values(v, gt.numpy())
  assert n == int((torch.nan_to_num(gt, nan=0.0) > 0).sum())
  assert abs(loss - float(ref)) <= 1e-6 * abs(float(ref))
  slopes = sref.pixel_slopes64(pred.detach().numpy(), gt.numpy()) / n
  assert float(np.abs(slopes - pred.grad.double().numpy()).max()) <= 3e-7 * float(np.abs(slopes).max())
  assert not bool(sref.valid(np.array([np.nan, -1.0, 0.0], dtype=np.float32)).any())
