"""The fp64 photometric reference (photometric_ref.py) against the oracle it restates, on the CPU: the GPU chain tests are only
as good as it is."""
import pytest
import torch

import photometric_ref as pr
from conftest import Golden, GOLDEN_CASES


def _inputs(B, H, W, seed, dmax):
  g = torch.Generator().manual_seed(seed)
  return torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g), torch.rand(B, 1, H, W, generator=g) * dmax


CASES = [(2, 37, 61, 20.0), (1, 96, 256, 60.0), (1, 9, 125, 125.0), (3, 2, 2, 2.0)]


@pytest.mark.parametrize("B,H,W,dmax", CASES)
def test_reference_in_float32_is_the_oracle(B, H, W, dmax):
  """Run in float32 on the oracle's decisions, the reference gives the oracle's bits: warped image, mask, loss map, masked sum
  and mean.  Its gradient is autograd through the explicit bilinear form rather than grid_sample's backward kernel, so it
  agrees to fp32 rounding, not bits: within 16 u of the gradient's own error scale."""
  left, right, pred = _inputs(B, H, W, seed=H + W, dmax=dmax)
  o = pr.oracle32(left, right, pred)
  dec = pr.decisions(left, right, pred)
  r = pr.chain(left, right, pred, dec, torch.float32)
  assert torch.equal(r["warped"], o["warped"]) and torch.equal(dec["mask"], o["mask"]) and torch.equal(r["total"], o["total"])
  assert r["count"] == o["count"] and torch.equal(r["sum"], o["sum"]) and torch.equal(r["mean"], o["mean"])
  r64 = pr.chain(left, right, pred, dec)
  wsc = pr.warp_scale(r64, H, W)
  scale = pr.grad_scale(r64, H, W, 1.0, 6 * wsc)
  err = (r["g_sum"].double() - o["g_sum"].double()).abs()
  assert bool((err <= 16 * pr.U * scale).all()), float((err / scale).max() / pr.U)


@pytest.mark.parametrize("B,H,W,dmax", CASES)
def test_reference_in_float64_is_the_oracle_to_fp32_rounding(B, H, W, dmax):
  """In float64 the reference is within the fp32 oracle's own rounding of it: the warped image, the loss map and the gradient
  within K u of their error scales (the K of tests/test_gpu_photometric_chain.py), the mean within 2^-20 relative.  The decision
  band is a share under 2^-21 * W of the pixels (its width over the coordinate's spacing)."""
  left, right, pred = _inputs(B, H, W, seed=H + W, dmax=dmax)
  o = pr.oracle32(left, right, pred)
  dec = pr.decisions(left, right, pred)
  r = pr.chain(left, right, pred, dec)
  wsc = pr.warp_scale(r, H, W)
  assert bool(((o["warped"].double() - r["warped"]).abs() <= 6 * pr.U * wsc).all())
  msc = pr.map_scales(r, H, W, wscale=6 * wsc)
  assert bool(((o["total"].double() - r["total"]).abs() <= 16 * pr.U * msc["total"]).all())
  assert abs(float(o["mean"]) - float(r["mean"])) <= 2.0 ** -20 * abs(float(r["mean"]))
  for which, gs in (("g_sum", 1.0), ("g_mean", 1.0 / r["count"])):
    scale = pr.grad_scale(r, H, W, gs, 6 * wsc)
    err = (o[which].double() - r["g_sum"] * gs).abs()
    assert bool((err <= 32 * pr.U * scale).all()), (which, float((err / scale).max() / pr.U))
  assert float(dec["band"].float().mean()) <= 2.0 ** -21 * W + 1e-12


def test_all_invalid_reference_is_nan_with_a_zero_gradient():
  """no valid pixel: the reference's loss is 0 / 0 (NaN) and its gradient exactly 0 (what the kernels must give too)"""
  left, right, _ = _inputs(2, 9, 61, seed=3, dmax=1.0)
  pred = torch.arange(61, dtype=torch.float32).view(1, 1, 1, 61).expand(2, 1, 9, 61) + 2.0
  o = pr.oracle32(left, right, pred)
  r = pr.chain(left, right, pred, pr.decisions(left, right, pred))
  assert o["count"] == 0 and r["count"] == 0
  assert bool(torch.isnan(o["mean"])) and bool(torch.isnan(r["mean"]))
  assert bool((o["g_mean"] == 0).all()) and bool((r["g_mean"] == 0).all()) and bool((r["g_sum"] == 0).all())


def test_decisions_at_the_mask_and_clip_limits():
  """x - d exactly 0 or W is valid (the inclusive test on nx), one fp32 step beyond is not unless nx rounds back onto -1 / 1;
  x - d - 1/2 exactly 0 or W - 1 is clipped (borders count as clipped: zero gradient)"""
  W, H = 64, 4
  x = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W).expand(1, 1, H, W)
  left = right = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(0))
  for pred, valid in ((x, True), (x - W, True), (x + 1e-3, False), (x - W - 1e-3, False)):
    assert bool((pr.decisions(left, right, pred)["mask"] == valid).all())
  for pred in (x - 0.5, x - W + 0.5):
    dec = pr.decisions(left, right, pred)
    assert bool(dec["cx"].all())
    left_, right_ = left, right
    o = pr.oracle32(left_, right_, pred)
    r = pr.chain(left_, right_, pred, dec)
    # clipped everywhere: only the smoothness and the mean term reach pred, as in the oracle
    assert float((o["g_sum"].double() - r["g_sum"]).abs().max()) <= 1e-6


def _loss_cases():
  """the fixtures that keep the refined disparity whole (the loss's input), with the loss and its map"""
  out = []
  for case in GOLDEN_CASES:
    gold = Golden(case)
    if gold.has("train/loss_total") and "full__train/pred_refined" in gold.z and "full__train/loss_total" in gold.z:
      out.append(case)
  return out


@pytest.mark.parametrize("case", _loss_cases())
def test_reference_reproduces_the_golden_loss(case):
  """the reference fixtures' adaptation loss (the reference's own monodepth loss of its refined disparity, tests/golden/):
  the float32 reference to the fixture's fp32 loss within 2 ulp (another torch build's reduction order), the float64 one
  within 2^-20 relative; the fixture's loss map to the float32 one within 4 ulp of the map's largest value"""
  gold = Golden(case)
  from adaptive_stereo.utils import synthetic as syn
  m = gold.meta
  left, right = syn.stereo_pair(m["B"], m["H"], m["W"], seed=1)
  exp = [float(v) for v in gold.z["sum__left"].reshape(-1)]
  assert all(abs(a - b) <= 1e-9 * max(1.0, abs(b)) for a, b in zip(syn.checksum(left), exp))
  pred = gold.full("train/pred_refined")
  dec = pr.decisions(left, right, pred)
  r32 = pr.chain(left, right, pred, dec, torch.float32)
  r64 = pr.chain(left, right, pred, dec)
  loss = gold.scalar("train/loss")
  assert abs(float(r32["mean"]) - loss) <= 2 * 2.0 ** -23 * abs(loss)
  assert abs(float(r64["mean"]) - loss) <= 2.0 ** -20 * abs(loss)
  tot = gold.full("train/loss_total")
  assert float((r32["total"] - tot).abs().max()) <= 4 * 2.0 ** -24 * float(tot.abs().max())


def test_smoothness_band_allowance_is_what_the_mean_rounding_can_change():
  """The smoothness band's allowance against the one way the band is reached: a per-image mean summed in fp64 and rounded once
  (as the kernels do) instead of the oracle's fp32 mean.  Vertical neighbours one ulp apart in pred make the band.  The signs
  taken with that mean differ from the oracle's only on band edges and only as 0 against +-1; the fp64 gradient on them moves by
  at most the allowance; off the band's pixels the allowance (its per-image mean part) is under 1e-3 of the rounding bound."""
  B, H, W = 2, 16, 64
  g = torch.Generator().manual_seed(2)              # (a seed where the two means round apart in both images)
  left, right = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
  pred = torch.rand(B, 1, H, W, generator=g) * 20
  pred[..., 1::2, :] = torch.nextafter(pred[..., 0::2, :], torch.full_like(pred[..., 0::2, :], 1e9))
  dec = pr.decisions(left, right, pred)
  ref = pr.chain(left, right, pred, dec)
  den_k = (pred.double().sum((2, 3), keepdim=True) * (1.0 / (H * W))).float() + 1e-7
  nd = pred / den_k
  dk = dict(dec, sx_sign=torch.sign(nd[..., :-1] - nd[..., 1:]), sy_sign=torch.sign(nd[..., :-1, :] - nd[..., 1:, :]))
  differ = [dk[k] != dec[k] for k in ("sx_sign", "sy_sign")]
  assert int(differ[0].sum() + differ[1].sum()) > 0                       # the inputs reach the band
  assert not bool((differ[0] & ~dec["sx_band"]).any()) and not bool((differ[1] & ~dec["sy_band"]).any())
  assert not bool((dk["sx_sign"] * dec["sx_sign"] < 0).any()) and not bool((dk["sy_sign"] * dec["sy_sign"] < 0).any())
  moved = (pr.chain(left, right, pred, dk)["g_sum"] - ref["g_sum"]).abs()
  allow = pr.smooth_band_allowance(ref, dec, 1.0)
  assert bool((moved <= allow * (1 + 1e-9)).all())
  near = torch.zeros_like(allow, dtype=torch.bool)
  near[..., :-1] |= dec["sx_band"]; near[..., 1:] |= dec["sx_band"]
  near[..., :-1, :] |= dec["sy_band"]; near[..., 1:, :] |= dec["sy_band"]
  o = pr.oracle32(left, right, pred)
  wsc = pr.warp_scale(ref, H, W)
  bound = torch.maximum(4 * (o["g_sum"].double() - ref["g_sum"]).abs(), 32 * pr.U * pr.grad_scale(ref, H, W, 1.0, 6 * wsc))
  assert bool((allow[~near] <= 1e-3 * bound[~near]).all())
