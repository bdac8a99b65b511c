"""Supervised training on the GPU: the kernels of csrc/supervised.hip and as_adam_step_lr through the C ABI, the supervised step
against the oracle, the captured step against eager stepping, the optimizer's state round trip, and train() end to end.

Kernel tests.  Every output is a slice of a larger buffer pre-filled with one NaN bit pattern (test_gpu_resample_fp64.Guarded):
after the launch no NaN is left inside and every word around it is bit-unchanged.
  as_khamis2_fwd   each loss within 1 float32 ulp of (float64 sum of the host's float32 per-pixel terms) / count — the kernel
                   divides in float64 and rounds once —, out4[2] the float32 sum of the two, the count exact.
  as_khamis2_bwd   G = scale x slope in float64 from the float32 inputs (supervised_ref.pixel_slopes64).  The kernel's expression
                   -scale * d / (2 sqrt(d * d + 4)) with scale = (g_a + g_b) / count passes K_SLOPE = 8 roundings: the sum and the
                   quotient of scale, d = gt - pred, d * d, + 4 (one rounding where the compiler fuses the two), the square root,
                   scale * d and the quotient (2 * x is exact).  g_pred0 is held to K_SLOPE 2^-24 |G|; g_coarse to
                   resample_ref.adjoint(G)'s own bound + K_SLOPE 2^-24 adjoint(|G|), exactly zero where that is zero.
  as_adam_step_lr  bit for bit as_adam_step at the same learning rate.

Three supervised steps against tests/supervised_ref.py (held to the reference by tests/test_supervised_ref_cpu.py), every step
from the same state, modelled on test_gpu_end_to_end.test_three_adaptation_steps_follow_the_oracle.  Per-tensor gradient bound:
2 x the worst row of tests/golden/reassociation_bound_supervised.json (tests/tools/reassociation_bound_supervised.py: what a
change of nothing but the convolutions' summation order does to the reference's own gradients of this step at this shape:
7.1e-3, a LeakyReLU kink crossed by a few of the 2,560 coarse voxels; the rule and its reason: test_gpu_end_to_end.py:33-40).
The 19 tensors whose gradient is analytically zero are held to the absolute allowance of an element of their layer's weight
gradient (tests/test_supervised_ref_cpu.py); every other tensor is compared.
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import GOLDEN_DIR, parity_note
from adaptive_stereo import _native as nat
from adaptive_stereo.adaptation import FusedClipAdam
from adaptive_stereo.training import SupervisedTrainer
from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
from adaptive_stereo.utils import synthetic as syn
from adaptive_stereo.utils.loss_functions import khamis_robust_loss_two_scale, khamis_robust_loss_multiscale
from oracle import stereo_oracle as orc
import resample_ref as rr
import supervised_ref as sref
from test_gpu_resample_fp64 import Guarded, _offset_copy

DEV = "cuda:0"
U = 2.0 ** -24
K_SLOPE = 8
BN_ATOL, BN_RTOL = 6e-5, 3e-4          # test_gpu_end_to_end's, for the same BatchNorm kernels
REASSOC = json.load(open(os.path.join(GOLDEN_DIR, "reassociation_bound_supervised.json")))
GRAD_BOUND = 2.0 * max(r["worst_tensor_rel_l2"] for c in REASSOC["cases"].values() for r in c["rows"].values())


def _gen(seed):
  return torch.Generator().manual_seed(seed)


def _maps(n, seed, holes=True):
  """(pred0, up, gt) of n values: predictions in 0 .. 40, gt = up + U(-6, 6) with zeros, negatives and NaN in between"""
  g = _gen(seed)
  pred0 = torch.rand(n, generator=g) * 40
  up = pred0 + torch.rand(n, generator=g) * 4 - 2
  gt = up + torch.rand(n, generator=g) * 12 - 6
  gt = gt.abs() + 0.25
  if holes and n > 1:
    gt[::3] = 0.0
    gt[1::7] = -gt[1::7]
    gt[2::11] = float("nan")
  return pred0, up, gt


def _khamis2_fwd(pred0, up, gt, off=0):
  n = pred0.numel()
  views = [_offset_copy(t, off) for t in (pred0, up, gt)]
  out4 = Guarded(4, off)
  ws = torch.empty(nat.load().as_khamis2_workspace(n), dtype=torch.float32, device=DEV)
  nat.call("as_khamis2_fwd", nat.ptr(views[0][0]), nat.ptr(views[1][0]), nat.ptr(views[2][0]), n, nat.ptr(out4.view), nat.ptr(ws),
           nat.stream())
  return out4.result("as_khamis2_fwd n=%d off=%d" % (n, off))


def _ulp32(x):
  return float(np.spacing(np.float32(abs(x))))


def _check_fwd(out4, pred0, up, gt, what):
  worst = 0.0
  losses = []
  for i, pred in enumerate((pred0, up)):
    ref, n = sref.loss_from_values(sref.pixel_values(pred.numpy(), gt.numpy()), gt.numpy())
    err = abs(float(out4[i]) - ref)
    ulp = _ulp32(ref) if ref != 0 else 0.0
    assert err <= ulp, "%s: loss %d = %r, expected %r (%.2f ulp)" % (what, i, float(out4[i]), ref, err / ulp if ulp else float("inf"))
    worst = max(worst, err / ulp if ulp else 0.0)
    losses.append(out4[i])
    assert float(out4[3]) == float(n), (what, float(out4[3]), n)
  assert float(out4[2]) == float(losses[0] + losses[1]), what          # (float32 tensors: a float32 sum)
  return worst


# ================================================================================================================ as_khamis2_fwd
@pytest.mark.parametrize("n", [1, 255, 257, 4099])
def test_khamis2_fwd_sizes_and_misaligned_bases(n):
  """one thread, one short of a workgroup, one over, and 17 workgroups with a ragged tail; every base 0 .. 3 floats past a
  16-byte boundary; zeros, negatives and NaN in the ground truth"""
  worst = 0.0
  for off in range(4):
    pred0, up, gt = _maps(n, seed=100 + n)
    worst = max(worst, _check_fwd(_khamis2_fwd(pred0, up, gt, off), pred0, up, gt, "n=%d off=%d" % (n, off)))
  parity_note("khamis2_fwd_n%d" % n, worst_ulp=worst)


def test_khamis2_fwd_one_valid_pixel_and_none():
  pred0, up, gt = _maps(4099, seed=7, holes=False)
  one = torch.zeros_like(gt); one[4098] = gt[4098]
  out4 = _khamis2_fwd(pred0, up, one)
  _check_fwd(out4, pred0, up, one, "one valid pixel")
  assert float(out4[3]) == 1.0 and float(out4[0]) > 0
  for none in (torch.zeros_like(gt), -gt, torch.full_like(gt, float("nan"))):
    out4 = _khamis2_fwd(pred0, up, none)
    assert [float(v) for v in out4] == [0.0, 0.0, 0.0, 1.0]


def test_khamis2_fwd_is_deterministic_and_refuses_bad_arguments():
  pred0, up, gt = _maps(4099, seed=8)
  a, b = _khamis2_fwd(pred0, up, gt), _khamis2_fwd(pred0, up, gt)
  assert torch.equal(a, b)
  lib = nat.load()
  assert lib.as_khamis2_workspace(0) == -1
  assert lib.as_khamis2_fwd(None, None, None, 4, None, None, nat.stream()) != 0
  assert b"as_khamis2_fwd" in lib.as_last_error()


# ================================================================================================================ as_khamis2_bwd
def _khamis2_bwd(pred0, up, gt, g3, B, H, W, h, w, gain, off=0):
  n = B * H * W
  views = [_offset_copy(t, off) for t in (pred0, up, gt)]
  out4 = torch.empty(4, device=DEV)
  ws = torch.empty(nat.load().as_khamis2_workspace(n), dtype=torch.float32, device=DEV)
  nat.call("as_khamis2_fwd", nat.ptr(views[0][0]), nat.ptr(views[1][0]), nat.ptr(views[2][0]), n, nat.ptr(out4), nat.ptr(ws),
           nat.stream())
  g3d = torch.tensor(g3, dtype=torch.float32).to(DEV)
  g_pred0, g_coarse = Guarded(n, off), Guarded(B * h * w, off)
  nat.call("as_khamis2_bwd", nat.ptr(views[0][0]), nat.ptr(views[1][0]), nat.ptr(views[2][0]), nat.ptr(g3d), nat.ptr(out4), B, H, W,
           h, w, float(gain), nat.ptr(g_pred0.view), nat.ptr(g_coarse.view), nat.stream())
  return (g_pred0.result("as_khamis2_bwd g_pred0").view(B, H, W), g_coarse.result("as_khamis2_bwd g_coarse").view(B, h, w),
          float(out4[3]))


def _check_bwd(B, h, w, H, W, gain, seed, off=0, g3=(0.75, -1.25, 0.5), gt_override=None):
  pred0, up, gt = _maps(B * H * W, seed)
  if gt_override is not None:
    gt = gt_override(gt)
  g_pred0, g_coarse, count = _khamis2_bwd(pred0, up, gt, g3, B, H, W, h, w, gain, off)
  assert count == max(int(sref.valid(gt.numpy()).sum()), 1)
  f = np.float32
  s0 = (float(f(g3[0])) + float(f(g3[2]))) / count          # (exact in float64)
  s1 = (float(f(g3[1])) + float(f(g3[2]))) / count
  G0 = torch.from_numpy(s0 * sref.pixel_slopes64(pred0.numpy(), gt.numpy())).view(B, H, W)
  G1 = torch.from_numpy(s1 * sref.pixel_slopes64(up.numpy(), gt.numpy())).view(B, H, W)
  r0 = rr.worst_ratio(g_pred0, G0, K_SLOPE * U * G0.abs())
  ref, bound, _ = rr.adjoint(G1, h, w, gain)
  allow = bound + K_SLOPE * U * rr.adjoint(G1.abs(), h, w, gain)[0]
  r1 = rr.worst_ratio(g_coarse, ref, allow)
  assert bool((g_coarse.double()[allow == 0] == 0).all()), "non-zero where no valid pixel reaches"
  return r0, r1, g_pred0, g_coarse


BWD_SHAPES = [(2, 10, 17, 75, 131, 8.0)] + [(2,) + s for s in rr.ONE + rr.TALL + rr.CHUNK_ONE] + [(2, 3, 2, 5, 9, 4.5)]


@pytest.mark.parametrize("shape", BWD_SHAPES, ids=lambda s: "%dx%d_to_%dx%d" % s[1:5])
def test_khamis2_bwd_against_fp64(shape):
  """the ragged production shape with the head's gain (8, not 131 / 17), a single coarse pixel, more than 256 footprint rows (no
  row-weight table), one coarse column per workgroup, a row shorter than a wave; bases off a 16-byte boundary"""
  B, h, w, H, W, gain = shape
  worst = (0.0, 0.0)
  for off in (0, 1, 3):
    r0, r1, _, _ = _check_bwd(B, h, w, H, W, gain, seed=31 + off, off=off)
    assert r0 <= 1.0 and r1 <= 1.0, (shape, off, r0, r1)
    worst = (max(worst[0], r0), max(worst[1], r1))
  parity_note("khamis2_bwd_%dx%d_to_%dx%d" % shape[1:5], g_pred0_over_bound=worst[0], g_coarse_over_bound=worst[1])


def test_khamis2_bwd_full_kitti_size():
  """(24, 78) <- (375, 1242) at two pairs: 16 coarse columns per workgroup with a ragged last chunk, the element-wise part on
  its grid-stride loop (931,500 pixels over 2,048 workgroups)"""
  r0, r1, _, _ = _check_bwd(2, 24, 78, 375, 1242, 16.0, seed=41)
  parity_note("khamis2_bwd_24x78_to_375x1242", g_pred0_over_bound=r0, g_coarse_over_bound=r1)
  assert r0 <= 1.0 and r1 <= 1.0


def test_khamis2_bwd_without_a_valid_pixel_is_all_zero():
  for kill in (lambda gt: torch.zeros_like(gt), lambda gt: torch.full_like(gt, float("nan"))):
    _, _, g_pred0, g_coarse = _check_bwd(2, 10, 17, 75, 131, 8.0, seed=51, gt_override=kill)
    assert float(g_pred0.abs().max()) == 0.0 and float(g_coarse.abs().max()) == 0.0


def test_khamis2_bwd_refuses_a_ratio_beyond_the_span():
  """as as_upsample_bilinear_bwd does (test_gpu_resample_fp64): error return, nothing written"""
  lib = nat.load()
  z = torch.zeros(400, device=DEV)
  g3, out4 = torch.ones(3, device=DEV), torch.ones(4, device=DEV)
  g_pred0, g_coarse = Guarded(400), Guarded(1)
  rc = lib.as_khamis2_bwd(nat.ptr(z), nat.ptr(z), nat.ptr(z), nat.ptr(g3), nat.ptr(out4), 1, 1, 400, 1, 1, 400.0,
                          nat.ptr(g_pred0.view), nat.ptr(g_coarse.view), nat.stream())
  torch.cuda.synchronize()
  msg = lib.as_last_error().decode()
  assert rc != 0 and "as_khamis2_bwd" in msg and "scale factor" in msg, msg
  assert g_pred0.untouched() and g_coarse.untouched()


# =============================================================================================================== as_adam_step_lr
@pytest.mark.parametrize("n", [1, 255, 257, 4099])
def test_adam_step_lr_is_bit_for_bit_adam_step(n):
  g = _gen(60 + n)
  p, grad, m, v = (torch.rand(n, generator=g) - 0.5 for _ in range(4))
  v = v.abs()
  worst_cases = 0
  for lr in (5e-5, 1.2345678e-3):
    lr_dev = torch.full((1,), lr, dtype=torch.float32, device=DEV)
    for scale in (None, torch.full((1,), 0.37, device=DEV)):
      for step, step_dev in ((3, None), (1, torch.full((1,), 5.0, device=DEV))):
        outs = []
        for name in ("as_adam_step", "as_adam_step_lr"):
          bufs = [Guarded(n, 1) for _ in range(3)]
          for b, t in zip(bufs, (p, m, v)):
            b.view.copy_(t)
          gd = grad.to(DEV)
          lr_arg = lr if name == "as_adam_step" else nat.ptr(lr_dev)
          nat.call(name, nat.ptr(bufs[0].view), nat.ptr(gd), nat.ptr(bufs[1].view), nat.ptr(bufs[2].view), n, nat.ptr(scale),
                   lr_arg, 0.9, 0.999, 1e-8, step, nat.ptr(step_dev), nat.stream())
          outs.append([b.result(name) for b in bufs])
        for a, b in zip(*outs):
          assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert not torch.equal(outs[0][0], p)          # (the step did move the parameters)
        worst_cases += 1
  assert worst_cases == 8
  lib = nat.load()
  assert lib.as_adam_step_lr(None, None, None, None, 4, None, None, 0.9, 0.999, 1e-8, 1, None, nat.stream()) != 0


# ========================================================================================================= the supervised step
def build(meta, seed=123):
  fnet = FeatureExtractorNetwork(meta["k"])
  snet = StereoNet(meta["k"], 1, meta["s"], maxdisp=meta["maxdisp"])
  fnet.load_state_dict(syn.synthetic_state_dict(fnet.state_dict(), seed=seed), strict=True)
  snet.load_state_dict(syn.synthetic_state_dict(snet.state_dict(), seed=seed, logit_gain=meta["gain"]), strict=True)
  return fnet.to(DEV), snet.to(DEV)


META = dict(k=3, s=0, maxdisp=64, gain=5.0)
B_, H_, W_ = 2, 64, 160
_BATCHES = {}


def batch(seed):
  """(left, right, gt) on the CPU, computed once: gt from the oracle's eval-mode prediction at the synthetic weights"""
  if seed not in _BATCHES:
    left, right = syn.stereo_pair(B_, H_, W_, seed=seed, disparities=(4.0, 7.0))
    fnet, snet = FeatureExtractorNetwork(3), StereoNet(3, 1, 0, maxdisp=64)
    fsd = syn.synthetic_state_dict(fnet.state_dict(), seed=123)
    ssd = syn.synthetic_state_dict(snet.state_dict(), seed=123, logit_gain=5.0)
    pred = orc.forward_only(fsd, ssd, left, right, 3, 0, 64)[0]["pred_disp_l/0"]
    _BATCHES[seed] = (left, right, sref.ground_truth(pred, 97))
  return _BATCHES[seed]


def on_device(seed):
  return tuple(t.to(DEV) for t in batch(seed))


def test_two_scale_loss_node_equals_the_composed_loss():
  """khamis_robust_loss_two_scale against khamis_robust_loss_multiscale + autograd on the same network outputs: the losses to
  two ulp of each (both kernels sum the same float32 terms in float64; they differ in how often the quotient is rounded),
  the gradients that reach the refined map and the soft-argmax output to the kernels' own bounds; without the stashed
  low-resolution map the function is the composed one."""
  fnet, snet = build(META)
  left, right, gt = on_device(41)
  fnet.train(); snet.train()
  out = snet(left, *fnet.forward_pair(left, right), "l")
  up = out["pred_disp_l/3"]
  coarse = up._as_coarse
  assert tuple(coarse.shape) == (B_, H_ // 8, W_ // 8) and up._as_coarse_gain == 8.0
  pred0 = out["pred_disp_l/0"].detach().requires_grad_(True)
  low = coarse.detach().requires_grad_(True)
  from adaptive_stereo import hip_ops
  up2 = hip_ops.UpsampleBilinearFn.apply(low, H_, W_, 8.0)
  assert torch.equal(up2, up)
  up2._as_coarse, up2._as_coarse_gain = low, 8.0
  inputs = {"gt_disp_l/0": gt}
  fused = khamis_robust_loss_two_scale(inputs, {"pred_disp_l/0": pred0, "pred_disp_l/3": up2}, 0, 3, 0)
  assert set(fused) == {"total_loss", "khamis_robust_loss/0", "khamis_robust_loss/3"}
  fused["total_loss"].backward()
  g_fused = (pred0.grad.clone(), low.grad.clone())
  pred0.grad = low.grad = None
  up3 = hip_ops.UpsampleBilinearFn.apply(low, H_, W_, 8.0)
  composed = khamis_robust_loss_multiscale(inputs, {"pred_disp_l/0": pred0, "pred_disp_l/3": up3}, scales=[0, 3], gt_disp_scale=0)
  composed["total_loss"].backward()
  for name in ("khamis_robust_loss/0", "khamis_robust_loss/3"):
    # (the single-scale kernel rounds the float64 sum and then the quotient: 1.5 ulp at worst; the fused one rounds once)
    assert abs(float(fused[name]) - float(composed[name])) <= 2 * _ulp32(float(composed[name])), name
  assert float(fused["total_loss"]) == float(fused["khamis_robust_loss/0"] + fused["khamis_robust_loss/3"])
  assert float((g_fused[0] - pred0.grad).abs().max()) <= 2 * K_SLOPE * U * float(pred0.grad.abs().max())
  _, bound, _ = rr.adjoint(torch.zeros(B_, H_, W_) + float(pred0.grad.abs().max()), H_ // 8, W_ // 8, 8.0)
  assert float((g_fused[1] - low.grad).abs().max()) <= 2 * float(bound.max())
  # no stash: the composed path
  plain = khamis_robust_loss_two_scale(inputs, {"pred_disp_l/0": pred0.detach(), "pred_disp_l/3": up3.detach()}, 0, 3, 0)
  assert float(plain["total_loss"]) == float(composed["total_loss"])


def test_three_supervised_steps_follow_the_oracle():
  """Three steps on three pairs, the learning rate halved before the third; every step compared from the same state (the oracle
  is loaded with the GPU's parameters and buffers), the carried state through a shadow optimizer that applies the oracle's
  Adam to the GPU's own gradients: see the module's docstring for the bounds."""
  fnet, snet = build(META)
  lr = 5e-5
  trainer = SupervisedTrainer(fnet, snet, lr=lr)
  names = ("stereo", "feature")
  nets = {"stereo": snet, "feature": fnet}
  w0 = {(n, name): p.detach().cpu().clone() for n in names for name, p in nets[n].named_parameters()}
  shadow = {key: t.clone() for key, t in w0.items()}
  shadow_state = {}
  zero_names = sref.zero_gradient_names(fnet.state_dict().keys(), snet.state_dict().keys())
  assert len(zero_names) == 19
  worst_rel, worst_shadow, worst_zero, compared = (0.0, ""), 0.0, 0.0, 0
  for step, seed in enumerate((41, 42, 43)):
    if step == 2:
      lr = lr / 2
      trainer.set_lr(lr)
    left, right, gt = batch(seed)
    fsd = {n: t.detach().cpu().clone() for n, t in fnet.state_dict().items()}
    ssd = {n: t.detach().cpu().clone() for n, t in snet.state_dict().items()}
    fp, sp = orc.make_params(fsd, True), orc.make_params(ssd, True)
    ref = sref.supervised_step(fp, sp, {}, left, right, gt, 3, 0, 64, lr=lr)
    got = trainer.step(left.to(DEV), right.to(DEV), gt.to(DEV))
    torch.cuda.synchronize()
    for name in ("total_loss", "khamis_robust_loss/0", "khamis_robust_loss/3"):
      rl, gl = float(ref[name]), float(got[name])
      assert abs(gl - rl) <= 2e-5 + 1e-5 * abs(rl), (step, name, gl, rl)
    groups = {"stereo": sp, "feature": fp}
    for mi, name, p, off, n in trainer.arena.entries:
      full = "%s.%s" % (names[mi], name)
      g_ref = groups[names[mi]][name].grad
      g = trainer.arena.grads[off:off + n].view(p.shape).detach().cpu()
      assert g_ref is not None, full
      if full in zero_names:
        wmax = float(groups[names[mi]][name[:-len("bias")] + "weight"].grad.abs().max())
        dev = float((g - g_ref).abs().max())
        worst_zero = max(worst_zero, dev / wmax)
        assert dev <= 1e-6 * META["gain"] + 2e-4 * wmax, (step, full, dev, wmax)
      else:
        rel = float((g - g_ref).double().norm() / g_ref.double().norm())
        worst_rel = max(worst_rel, (rel, "step %d %s" % (step, full)))
        assert rel <= GRAD_BOUND, (step, full, rel)
        compared += 1
      orc.adam_step(shadow[(names[mi], name)], g, shadow_state.setdefault((names[mi], name), {}), lr)
      dev = float((p.detach().cpu() - shadow[(names[mi], name)]).abs().max())
      worst_shadow = max(worst_shadow, dev)
      assert dev <= 2e-7 * (step + 1), (step, full, dev)
    assert trainer.optimizer.step_count == step + 1 and float(trainer.optimizer.step_dev) == step + 1.0
    for n_, net, ref_p in (("feature", fnet, fp), ("stereo", snet, sp)):
      sd = net.state_dict()
      assert set(sd.keys()) == set(ref_p.keys())
      for key, ref_t in ref_p.items():
        if key.endswith("num_batches_tracked"):
          assert int(sd[key]) == int(ref_t), (step, key)
        elif key.endswith(("running_mean", "running_var")):
          diff = (sd[key].detach().cpu() - ref_t).abs()
          assert bool((diff <= BN_ATOL + BN_RTOL * ref_t.abs()).all()), (step, n_, key, float(diff.max()))
  assert compared == 3 * 61
  for mi, listed in enumerate(trainer.arena.all_params):          # BasicBlock.conv2: never run, never moved
    for name, p, live in listed:
      if not live:
        assert p.grad is None and torch.equal(p.detach().cpu(), w0[(names[mi], name)]), name
  moved = sum(float((p.detach().cpu() - w0[(n, name)]).double().pow(2).sum()) for n in names
              for name, p in nets[n].named_parameters()) ** 0.5
  parity_note("three_supervised_steps", worst_grad_rel_l2=worst_rel[0], worst_tensor=worst_rel[1], bound=GRAD_BOUND,
              worst_zero_gradient_over_weight_gradient=worst_zero, worst_shadow_optimizer_deviation=worst_shadow, moved_norm=moved)
  assert moved > 100 * lr, moved


def _state(trainer):
  return {name: t.detach().clone() for name, t in trainer._state_tensors().items()}


def _same(a, b):
  assert a.keys() == b.keys()
  for name in a:
    x, y = a[name], b[name]
    assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), name


def test_captured_replay_equals_eager_stepping():
  """Two trainers from the same weights, one stepping eagerly, one replaying the graph captured before its first step: after
  every one of three steps (a set_lr between the second and the third) losses, parameters, moments, step count and BatchNorm
  buffers are bit-identical and one graph exists; capture() itself changes nothing; a batch of another size runs eagerly on
  both and the graph replays correctly after it."""
  eager = SupervisedTrainer(*build(META), lr=5e-5)
  graph = SupervisedTrainer(*build(META), lr=5e-5)
  before = _state(graph)
  first = on_device(41)
  outer, side, x = torch.cuda.CUDAGraph(), torch.cuda.Stream(), torch.zeros(4, device=DEV)
  torch.cuda.synchronize()
  with torch.cuda.graph(outer, stream=side, capture_error_mode="thread_local"):
    x.add_(1.0)
    with pytest.raises(RuntimeError, match="already being captured"):          # refused before anything is issued
      graph.capture(*first)
  assert graph.graph_count() == 0
  graph.capture(*first)
  torch.cuda.synchronize()
  _same(_state(graph), before)
  assert graph.graph_count() == 1 and eager.graph_count() == 0 and graph.optimizer.step_count == 0
  seeds = (41, 42, 43)
  for step, seed in enumerate(seeds):
    if step == 2:
      eager.set_lr(1.25e-5); graph.set_lr(1.25e-5)
    a, b = eager.step(*on_device(seed)), graph.step(*on_device(seed))
    torch.cuda.synchronize()
    for name in ("total_loss", "khamis_robust_loss/0", "khamis_robust_loss/3"):
      assert float(a[name]) == float(b[name]), (step, name)
    assert torch.equal(a["outputs"]["pred_disp_l/0"], b["outputs"]["pred_disp_l/0"])
    _same(_state(eager), _state(graph))
    assert graph.graph_count() == 1 and graph.optimizer.step_count == step + 1
  small = tuple(t[:1].contiguous() for t in on_device(42))
  a, b = eager.step(*small), graph.step(*small)
  assert float(a["total_loss"]) == float(b["total_loss"]) and graph.graph_count() == 1
  _same(_state(eager), _state(graph))
  a, b = eager.step(*on_device(43)), graph.step(*on_device(43))
  torch.cuda.synchronize()
  assert float(a["total_loss"]) == float(b["total_loss"])
  _same(_state(eager), _state(graph))
  ins = graph.graph_inputs()
  assert torch.equal(ins[0], on_device(43)[0]) and torch.equal(ins[2], on_device(43)[2])


def test_optimizer_state_round_trip(tmp_path):
  """load_state_dict(state_dict()) followed by a step equals the uninterrupted run bit for bit; the file loads into
  torch.optim.Adam over the same parameter groups."""
  fnet, snet = build(META)
  trainer = SupervisedTrainer(fnet, snet, lr=5e-5, clip_grad_norm=True)
  for seed in (41, 42):
    trainer.step(*on_device(seed))
  trainer.set_lr(2.5e-5)
  sd = trainer.optimizer.state_dict()
  path = str(tmp_path / "adam.pth")
  torch.save(sd, path)
  snap = _state(trainer)
  trainer.step(*on_device(43))
  torch.cuda.synchronize()
  uninterrupted = _state(trainer)
  with torch.no_grad():
    for name, t in trainer._state_tensors().items():
      t.copy_(snap[name])
  opt = trainer.optimizer
  opt.exp_avg.fill_(7.0); opt.exp_avg_sq.fill_(7.0); opt.step_dev.fill_(99.0); opt.step_count = 99
  opt.set_lr(1.0)
  opt.load_state_dict(torch.load(path, map_location="cpu"))
  assert opt.step_count == 2 and float(opt.step_dev) == 2.0 and opt.lr == 2.5e-5 and float(opt.lr_dev) == float(np.float32(2.5e-5))
  trainer.step(*on_device(43))
  torch.cuda.synchronize()
  _same(_state(trainer), uninterrupted)
  # torch.optim.Adam over (stereo_net, feature_net): train.py:165
  cpu = [[p.detach().cpu().clone().requires_grad_(True) for p in net.parameters()] for net in (snet, fnet)]
  adam = torch.optim.Adam([{"params": cpu[0]}, {"params": cpu[1]}], lr=1.0)
  adam.load_state_dict(torch.load(path, map_location="cpu"))
  assert adam.param_groups[0]["lr"] == 2.5e-5 and len(adam.state) == len(sd["state"]) > 60
  first = next(iter(adam.state.values()))
  assert float(first["step"]) == 2.0 and first["exp_avg"].shape == first["exp_avg_sq"].shape
  # the default optimizer keeps the host learning rate and as_adam_step
  assert FusedClipAdam(trainer.arena, 1e-5).lr_dev is None


def test_loss_falls_on_a_repeated_batch():
  """ten steps on one batch at lr 5e-5: the total loss after them is strictly below the first (the reference, through
  tests/supervised_ref.py on the CPU at these weights, this batch and this learning rate: 10.21 -> 1.90, every step lower)"""
  trainer = SupervisedTrainer(*build(META), lr=5e-5)
  data = on_device(41)
  losses = [trainer.step(*data)["total_loss"].clone() for _ in range(11)]
  losses = [float(v) for v in losses]
  parity_note("loss_on_a_repeated_batch", first=losses[0], after_ten=losses[10])
  assert losses[10] < losses[0], losses


# ======================================================================================================================= train()
class ListDataset(torch.utils.data.Dataset):
  def __init__(self, samples):
    self.samples = samples

  def __len__(self):
    return len(self.samples)

  def __getitem__(self, i):
    return self.samples[i]


def _samples():
  out = []
  for i, seed in enumerate((41, 42, 43)):
    left, right, gt = batch(seed)
    for b in range(B_):
      out.append({"color_l/0": left[b], "color_r/0": right[b], "gt_disp_l/0": gt[b]})
  return out[:5]


def test_train_end_to_end(tmp_path):
  """train() on an injected dataset of 5 samples, batch 2 (a last batch of one: eager next to the captured step), two epochs,
  the learning rate halved after each: opt.json, the reference's checkpoint layout, the schedule in adam.pth, and final weights
  bit-identical to a hand-written loop of eager SupervisedTrainer.step calls on the same batches."""
  import train as train_module
  from torch.utils.data import DataLoader
  samples = _samples()
  lr = 5e-5
  opt = train_module.TrainOptions().parse([
      "--height", "64", "--width", "160", "--model_name", "run", "--log_dir", str(tmp_path), "--batch_size", "2",
      "--stereonet_k", "3", "--num_epochs", "2", "--scheduler_step_size", "1", "--num_workers", "0", "--no_shuffle",
      "--learning_rate", str(lr), "--log_frequency", "2"])

  class Writer(object):
    def __init__(self):
      self.scalars, self.images = [], []

    def add_scalar(self, name, value, step):
      self.scalars.append((name, step))

    def add_image(self, name, image, step):
      self.images.append((name, step))

  writer = Writer()
  trainer = train_module.train(opt, train_dataset=ListDataset(samples), val_dataset=ListDataset(samples[:2]), writer=writer)
  torch.cuda.synchronize()
  assert trainer.graph_count() == 1 and trainer.optimizer.step_count == 6
  log_path = os.path.join(str(tmp_path), "run")
  saved_opt = json.load(open(os.path.join(log_path, "opt.json")))
  assert saved_opt["learning_rate"] == lr and saved_opt["scheduler_step_size"] == 1 and "commit_hash" in saved_opt
  folder = os.path.join(log_path, "models", "weights_1")
  assert sorted(os.listdir(os.path.join(log_path, "models"))) == ["weights_1"]
  assert sorted(os.listdir(folder)) == ["adam.pth", "feature_net.pth", "stereo_net.pth"]
  adam = torch.load(os.path.join(folder, "adam.pth"), map_location="cpu")
  assert [g["lr"] for g in adam["param_groups"]] == [lr * 0.25, lr * 0.25]          # StepLR(1, 0.5) stepped after each epoch
  assert {name for name, _ in writer.scalars} >= {"total_loss", "khamis_robust_loss/0", "khamis_robust_loss/3", "EPE"}
  assert ("total_loss", 0) in writer.scalars and ("total_loss", 3) in writer.scalars and writer.images

  # the same run by hand: eager steps only
  torch.manual_seed(123)
  fnet = FeatureExtractorNetwork(3).cuda()
  snet = StereoNet(3, 1, 0).cuda()
  hand = SupervisedTrainer(fnet, snet, lr=lr)
  for epoch in range(2):
    for inputs in DataLoader(ListDataset(samples), 2, False):
      hand.step(inputs["color_l/0"].cuda(), inputs["color_r/0"].cuda(), inputs["gt_disp_l/0"].cuda())
    hand.set_lr(lr * 0.5 ** (epoch + 1))
  torch.cuda.synchronize()
  assert hand.graph_count() == 0
  for name, net in (("feature_net", fnet), ("stereo_net", snet)):
    sd = torch.load(os.path.join(folder, name + ".pth"), map_location="cpu")
    mine = net.state_dict()
    assert list(sd.keys()) == list(mine.keys())
    for key, t in sd.items():
      assert torch.equal(t, mine[key].detach().cpu()), (name, key)
  # and the checkpoint resumes: weights and optimizer state load back
  opt2 = train_module.TrainOptions().parse([
      "--height", "64", "--width", "160", "--model_name", "resumed", "--log_dir", str(tmp_path), "--batch_size", "2",
      "--stereonet_k", "3", "--num_epochs", "1", "--num_workers", "0", "--no_shuffle", "--load_weights_folder", folder,
      "--load_adam"])
  resumed = train_module.train(opt2, train_dataset=ListDataset(samples[:2]), val_dataset=ListDataset(samples[:2]), writer=writer)
  assert resumed.optimizer.step_count == 7
