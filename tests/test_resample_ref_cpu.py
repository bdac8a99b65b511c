"""tests/resample_ref.py held to torch on the CPU, so that the reference of tests/test_gpu_resample_fp64.py cannot drift with the
kernel it judges: F.interpolate in float32 (forward and autograd adjoint) and float32 emulations of the kernel's own order of
operations lie inside the bound at every shape the GPU file uses; F.interpolate in float64 (float64 coordinates) lies inside the
widened coordinate term alone, which is what checks the neighbouring-cell refinement; the weights sum to one; the adjoint
conserves the gradient's sum; and a float32 emulation of the backward's footprint() covers every non-zero entry of W."""
import pytest
import torch
import torch.nn.functional as F

import resample_ref as rr

IDS = ["%dx%d_to_%dx%d" % s[:4] for s in rr.ALL_SHAPES]


def _rnd(*shape, seed):
  return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1


def _interp(src, H, W, gain):
  return F.interpolate(src.unsqueeze(1), size=(H, W), mode="bilinear", align_corners=False).squeeze(1) * gain


@pytest.mark.parametrize("shape", rr.ALL_SHAPES, ids=IDS)
def test_aten_float32_is_inside_the_bound(shape):
  """forward and adjoint of F.interpolate in float32; worst ratios seen: forward 0.5 (coordinate term), backward 0.05"""
  h, w, H, W, gain = shape
  gain32 = torch.tensor(gain, dtype=torch.float32)
  src = _rnd(2, h, w, seed=1).float().requires_grad_(True)
  out = _interp(src, H, W, gain32)
  ref, bound, _ = rr.forward(src, H, W, gain)
  rf = rr.worst_ratio(out, ref, bound)
  g = _rnd(2, H, W, seed=2).float()
  out.backward(g)
  refb, boundb, _ = rr.adjoint(g, h, w, gain)
  rb = rr.worst_ratio(src.grad, refb, boundb)
  print("aten fp32 %s: forward %.3f backward %.3f of the bound" % (shape[:4], rf, rb))
  assert rf <= 1.0 and rb <= 1.0


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("shape", rr.ALL_SHAPES, ids=IDS)
def test_kernel_order_emulation_is_inside_the_bound(shape, fused):
  h, w, H, W, gain = shape
  src = _rnd(2, h, w, seed=3).float()
  out = rr.forward_kernel_order(src, H, W, gain, fused)
  ref, bound, _ = rr.forward(src, H, W, gain)
  r = rr.worst_ratio(out, ref, bound)
  print("kernel order %s fused=%d: %.3f of the bound" % (shape[:4], fused, r))
  assert r <= 1.0


@pytest.mark.parametrize("shape", rr.ALL_SHAPES, ids=IDS)
def test_aten_float64_is_inside_the_widened_coordinate_term(shape):
  """F.interpolate on float64 tensors computes the coordinates in float64: the only difference to the reference is the
  coordinate (half an ulp of the float32 product, the rounding of the float32 scale, and the cell where those cross an
  integer).  Allowance: the widened coordinate term, once, plus 64 * 2^-53 * mag of float64 noise — nothing else.  Without the
  neighbouring-cell marks of resample_ref.matrices this fails by factors of 3 to 23 at the production shapes."""
  h, w, H, W, gain = shape
  gain32 = float(torch.tensor(gain, dtype=torch.float32))
  src = _rnd(2, h, w, seed=4).float().double().requires_grad_(True)
  out = _interp(src, H, W, gain32)
  ref, bound, coord = rr.forward(src, H, W, gain, widen=True)
  mag = (bound - 2.0 * coord) / (rr.K_FWD * rr.U)
  rf = rr.worst_ratio(out, ref, coord + 64 * 2.0 ** -53 * mag)
  g = _rnd(2, H, W, seed=5).float().double()
  out.backward(g)
  refb, boundb, coordb = rr.adjoint(g, h, w, gain, widen=True)
  magb = (boundb - 2.0 * coordb) / (rr.k_bwd(h, w, H, W)[0] * rr.U)
  rb = rr.worst_ratio(src.grad, refb, coordb + 64 * 2.0 ** -53 * magb)
  print("aten fp64 %s: forward %.3f backward %.3f of the widened coordinate term" % (shape[:4], rf, rb))
  assert rf <= 1.0 and rb <= 1.0


@pytest.mark.parametrize("shape", rr.ALL_SHAPES, ids=IDS)
def test_weights_sum_to_one_and_the_adjoint_conserves_the_sum(shape):
  h, w, H, W, gain = shape
  for n, N in ((h, H), (w, W)):
    Wm, _ = rr.matrices(n, N)
    assert float((Wm.sum(1) - 1.0).abs().max()) <= 2.0 ** -52
    assert bool((Wm >= 0).all()) and int((Wm != 0).sum(1).max()) <= 2
  c = 0.7310585786300049
  src = torch.full((1, h, w), c, dtype=torch.float32)
  for fused in (False, True):
    out = rr.forward_kernel_order(src, H, W, gain, fused).double()
    exact = float(src[0, 0, 0]) * float(torch.tensor(gain, dtype=torch.float32))
    assert float((out - exact).abs().max()) <= 2 * 2.0 ** -23 * abs(exact), "constant source: more than 2 ulp"
  g = _rnd(2, H, W, seed=6)
  ref, _, _ = rr.adjoint(g, h, w, gain)
  g32 = float(torch.tensor(gain, dtype=torch.float32))
  assert abs(float(ref.sum()) - g32 * float(g.sum())) <= 1e-12 * g32 * float(g.abs().sum())


def _footprint_misses(n, N, tighten=0):
  """entries of W outside the float32 footprint -> (their weights, their coordinate allowance 2 E)"""
  Wm, E = rr.matrices(n, N)
  lo, hi = rr.footprint32(n, N, tighten)
  idx = torch.arange(N)[:, None]
  out = (Wm != 0) & ~((idx >= lo[None, :]) & (idx <= hi[None, :]))
  return Wm[out], 2.0 * E[out]


def _footprint_covers(n, N):
  return _footprint_misses(n, N)[0].numel() == 0


def _size_pairs():
  pairs = set()
  for h, w, H, W, _ in rr.ALL_SHAPES:
    pairs.update([(h, H), (w, W), (H, h), (W, w)])
  for n in range(1, 80):
    for N in range(1, 400, 7):
      pairs.add((n, N))
  pairs.update([(1, 1000), (1000, 1), (2, 679), (3, 1017), (1242, 155), (155, 1242), (4100, 50), (50, 4100), (1025, 1500)])
  return sorted(pairs)


def test_footprint_covers_every_contributing_fine_index():
  """footprint() in float32 against the reference's W: all shapes of the GPU file, every n < 80 with N < 400 in steps of 7, and
  the production and extreme ratios in both directions"""
  missed = [p for p in _size_pairs() if not _footprint_covers(*p)]
  assert not missed, missed[:10]


def test_footprint_slack_guards_only_weights_inside_the_coordinate_allowance():
  """Why a GPU test cannot tell footprint() from one with its slack of 1 removed and one index tighter: floor(lower) + 1 is the
  first index whose exact coordinate lies inside the tap's support, so all that the slack still catches are weights of a few ulp
  of the coordinate, which the reference does not pin (the other rounding of the coordinate gives them weight zero).  Over the
  sweep such entries exist (the slack is not idle), each inside its own coordinate allowance (2 E; at most half of it in this sweep); one index tighter still
  drops whole taps."""
  seen, worst = 0, 0.0
  for n, N in _size_pairs():
    w, allow = _footprint_misses(n, N, tighten=2)
    seen += w.numel()
    if w.numel():
      assert bool((allow > 0).all())
      worst = max(worst, float((w / allow).max()))
  assert seen > 0 and worst <= 1.0, (seen, worst)
  w, _ = _footprint_misses(78, 1242, tighten=3)
  assert w.numel() > 0 and float(w.max()) > 0.01
