"""The adaptation step's loss chain (as_photometric_chain_fwd / _bwd, csrc/photometric_rows.hip) and the row kernels' loss maps
(as_monodepth_loss_rows_fwd) against an fp64 reference that takes the fp32 oracle's discrete decisions (photometric_ref.py),
at the strip / column-block edges and at the inputs where the chain's branches decide: exact ties, the mask and clip limits,
pixels on the bilinear cells' edges, few or no valid pixels, constant and zero disparities.

Bounds.  Integer and discrete outputs (mask, count) are exact.  Every continuous element obeys

    |kernel - fp64| <= max(C * |oracle_fp32 - fp64|, K * u * scale),       u = 2^-24,

where scale is the element's own magnitude sum (photometric_ref.warp_scale / map_scales / grad_scale: the terms the fp32
arithmetic adds, with the SSIM terms' cancellation M / B2, M = E[x^2] + mu_x^2 + E[y^2] + mu_y^2 + 2 (E|xy| + |mu_x mu_y|)).
C = 4: the kernels and the oracle round the same formulas in a different order; K is stated per tensor below as the number of
roundings a term passes through.  Each tensor's worst ratio of error to bound is reported with parity_note.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import parity_note
import photometric_ref as pr
from adaptive_stereo import _native as nat
from adaptive_stereo import hip_ops as ops

DEV = "cuda:0"
U = pr.U
C = 4.0


def ratio(got, ref64, o32, scale, K, what, allow=0.0):
  """worst |got - ref64| / (max(C |o32 - ref64|, K u scale) + allow); asserts <= 1 and finite"""
  got = got.detach().cpu().double()
  assert got.shape == ref64.shape, (what, tuple(got.shape), tuple(ref64.shape))
  assert bool(torch.isfinite(got).all()), "%s: %d non-finite" % (what, int((~torch.isfinite(got)).sum()))
  err = (got - ref64).abs()
  bound = torch.maximum(C * (o32.double() - ref64).abs(), K * U * scale) + allow
  r = err / bound
  r = torch.where(err == 0, torch.zeros_like(r), r)
  worst = float(r.max())
  if worst > 1.0:
    i = int(r.flatten().argmax())
    raise AssertionError("%s: worst err / bound %.3f at flat %d (err %.3e, bound %.3e, got %.9g, fp64 %.9g, fp32 oracle %.9g); "
                         "%d of %d over" % (what, worst, i, float(err.flatten()[i]), float(bound.flatten()[i]),
                                            float(got.flatten()[i]), float(ref64.flatten()[i]), float(o32.flatten()[i]),
                                            int((r > 1).sum()), r.numel()))
  return worst


# ----------------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
  return torch.Generator().manual_seed(seed)


def _blocks(B, H, W, g, bs=4):
  """piecewise-constant image with dyadic values k/64 in bs x bs blocks [B,3,H,W]"""
  v = torch.randint(0, 64, (B, 3, (H + bs - 1) // bs, (W + bs - 1) // bs), generator=g).float() / 64
  return v.repeat_interleave(bs, 2).repeat_interleave(bs, 3)[..., :H, :W].contiguous()


def _shift(img, d):
  """right(x) = left(x + d), the last column repeated: a right image whose warp by disparity d gives the left one back"""
  return torch.cat([img[..., d:], img[..., -1:].expand(*img.shape[:-1], d)], dim=-1).contiguous()


def _xs(B, H, W):
  return torch.arange(W, dtype=torch.float32).view(1, 1, 1, W).expand(B, 1, H, W)


def make_inputs(family, B, H, W, seed=0):
  g = _gen(seed)
  rand_imgs = lambda: (torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g))
  xs = _xs(B, H, W)
  if family == "random":                                    # disparities inside the usual range, most samples valid
    left, right = rand_imgs()
    return left, right, torch.rand(B, 1, H, W, generator=g) * min(30.0, W / 3.0)
  if family == "disp_to_W":                                 # disparities up to W: about half the pixels invalid
    left, right = rand_imgs()
    return left, right, torch.rand(B, 1, H, W, generator=g) * W
  if family == "ties":
    # dyadic blocks, integer disparities 2 or 3 in blocks, the right image the left one shifted by 3: exact-zero L1 and
    # smoothness differences, windows with x == y (SSIM raw exactly 0, where the clamp passes the gradient)
    left = _blocks(B, H, W, g)
    right = _shift(left, 3)
    pred = 2.0 + (torch.rand(B, 1, (H + 7) // 8, (W + 7) // 8, generator=g) < 0.7).float()
    pred = pred.repeat_interleave(8, 2).repeat_interleave(8, 3)[..., :H, :W].contiguous()
    return left, right, pred
  if family == "near_identical":
    # dark ramps (slope 2^-14 per column, so the warp's slope is not zero) and a disparity of 3: the warped image is the ramp
    # exactly (power-of-two extents: exact sample coordinates), the left image is it + 2^-20.  Near-identical windows with
    # mu ~ 0.01 (delta^2 / mu^2 < u): fp32 n/d lands on either side of 1 by rounding, and where it lands above, the reference
    # clamps (no gradient).  Dark, because the clamp's gradient is ~ delta / C2 while the SSIM terms' rounding grows with
    # mu^2 / C2: this is where a kernel that ignored the clamp would stand out of the rounding
    b = torch.randint(4, 16, (B, 3, 1, 1), generator=g).float() / 1024
    x = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W)
    right = (b + x * 2.0 ** -14).expand(B, 3, H, W).contiguous()
    left = (b + (x - 3.5).clamp(min=0) * 2.0 ** -14 + 2.0 ** -20).expand(B, 3, H, W).contiguous()
    return left, right, torch.full((B, 1, H, W), 3.0)
  if family == "mask_clip":
    # per pixel one of: x - d exactly 0 or W and one ulp either side; x - d - 1/2 exactly 0 or W - 1 (the clip, zero gradient);
    # beyond the image on either side; half-integer disparities (samples on pixel centres: the floor picks the cell)
    left, right = rand_imgs()
    x = xs
    W_ = float(W)
    up = lambda t: torch.nextafter(t, torch.full_like(t, math.inf))
    dn = lambda t: torch.nextafter(t, torch.full_like(t, -math.inf))
    cands = [x, up(x), dn(x), x - W_, up(x - W_), dn(x - W_), x - 0.5, x - W_ + 0.5, up(x - 0.5), dn(x - W_ + 0.5),
             x + 1 + torch.rand(B, 1, H, W, generator=g) * 5, x - W_ - 1 - torch.rand(B, 1, H, W, generator=g) * 5,
             torch.randint(0, W, (B, 1, H, W), generator=g).float() + 0.5, -torch.randint(0, 4, (B, 1, H, W), generator=g).float() - 0.5]
    pick = torch.randint(0, len(cands), (B, 1, H, W), generator=g)
    pred = torch.zeros(B, 1, H, W)
    for i, c in enumerate(cands):
      pred = torch.where(pick == i, c, pred)
    return left, right, pred.contiguous()
  if family == "one_valid":                                 # every sample left of the image but one
    left, right = rand_imgs()
    pred = xs + 10.0
    pred = pred.clone()
    pred[0, 0, H // 2, W // 2] = 0.25
    return left, right, pred.contiguous()
  if family == "one_image_invalid":
    left, right = rand_imgs()
    pred = torch.rand(B, 1, H, W, generator=g) * min(30.0, W / 3.0)
    pred[-1] = xs[-1] + 3.0
    return left, right, pred.contiguous()
  if family == "all_invalid":
    left, right = rand_imgs()
    return left, right, (xs + 1.0 + torch.rand(B, 1, H, W, generator=g)).contiguous()
  if family == "const_pred":                                # zero smoothness differences: only the mean + 1e-7 term is left
    left, right = rand_imgs()
    return left, right, torch.full((B, 1, H, W), 7.25)
  if family == "zero_pred":
    left, right = rand_imgs()
    return left, right, torch.zeros(B, 1, H, W)
  if family == "tiny_pred":                                 # mean disparity ~ 5e-7: the + 1e-7 of the normalisation matters
    left, right = rand_imgs()
    return left, right, torch.rand(B, 1, H, W, generator=g) * 1e-6
  raise ValueError(family)


# ----------------------------------------------------------------------------------------------------------------------------
# the live chain
# ----------------------------------------------------------------------------------------------------------------------------
def run_chain(left, right, pred):
  """-> warped, mask, out4, g_pred for g_mean = 1 (MaskedPhotometricFn, the one-GPU step), g_pred for g_sum = 1 (the C ABI
  with a NULL g_mean, what a data-parallel rank back-propagates)"""
  B, _, H, W = left.shape
  lib = nat.load()
  l, r = left.to(DEV), right.to(DEV)
  p = pred.to(DEV).requires_grad_(True)
  mean, lsum, count, warped, mask = ops.MaskedPhotometricFn.apply(p, l, r, pr.SW)
  mean.backward()
  g_mean_pred = p.grad.detach().clone()
  pd = pred.to(DEV)
  ws_f = torch.empty(lib.as_photometric_chain_workspace(B, H, W), device=DEV)
  ws_b = torch.empty(lib.as_photometric_chain_workspace(B, H, W), device=DEV)
  w2 = torch.empty_like(r)
  m2 = torch.empty(B, 1, H, W, dtype=torch.uint8, device=DEV)
  out4 = torch.full((4,), float("nan"), device=DEV)
  g_sum = torch.ones(1, device=DEV)
  g2 = torch.full_like(pd, float("nan"))
  nat.call("as_photometric_chain_fwd", nat.ptr(pd), nat.ptr(l), nat.ptr(r), B, H, W, pr.SW, nat.ptr(w2), nat.ptr(m2), nat.ptr(out4),
           nat.ptr(ws_f), nat.stream())
  nat.call("as_photometric_chain_bwd", nat.ptr(g_sum), None, nat.ptr(out4), nat.ptr(pd), nat.ptr(l), nat.ptr(r), B, H, W, pr.SW,
           nat.ptr(g2), nat.ptr(ws_b), nat.ptr(ws_f), nat.stream())
  torch.cuda.synchronize()
  # the two paths run the same launches
  assert torch.equal(w2, warped) and torch.equal(m2, mask)
  return dict(warped=warped.cpu(), mask=mask.cpu(), out4=out4.cpu(), mean=float(mean), g_mean=g_mean_pred.cpu(), g_sum=g2.cpu())


def check_chain(tag, left, right, pred, band_share_max=None):
  B, _, H, W = left.shape
  dec = pr.decisions(left, right, pred)
  o32 = pr.oracle32(left, right, pred)
  ref = pr.chain(left, right, pred, dec)
  got = run_chain(left, right, pred)
  n = ref["count"]

  # discrete outputs: exact
  assert torch.equal(got["mask"].bool(), dec["mask"]) and torch.equal(o32["mask"], dec["mask"])
  assert float(got["out4"][1]) == n and float(got["out4"][3]) == n

  notes = dict(count=n, pixels=B * H * W, band=int(dec["band"].sum()))
  # warped: the taps times the bilinear weights plus the slope times the sample coordinate's roundings (warp_scale): each of
  # the two products and three fma / additions of the sum rounds once, K = 6
  wsc = pr.warp_scale(ref, H, W)
  notes["warped"] = ratio(got["warped"], ref["warped"], o32["warped"], wsc, 6, tag + " warped")
  # what follows reads the warped image the kernel made, not the exact one: its deviation (bounded just above) enters the
  # loss map's and the gradient's scales as an input perturbation, twice the larger of the kernel's and the oracle's, in u
  dy = 2 * torch.maximum((got["warped"].double() - ref["warped"]).abs(), (o32["warped"].double() - ref["warped"]).abs()) / U

  # out4 = (sum, count, mean, count).  The sum of the masked fp32 loss map: each element within K_t u scale_total of fp64
  # (K_t = 16: ~10 roundings between the pooled moments and the map, the warped image's own error carried in the scale),
  # accumulated in fp64 and rounded once (u |sum|); the mean = fl(sum) / fl(count), two more roundings.
  msc = pr.map_scales(ref, H, W, wscale=dy)
  esum = float((16 * U * msc["total"])[dec["mask"]].sum()) + U * abs(float(ref["sum"]))
  e32 = abs(float(o32["sum"]) - float(ref["sum"]))
  bsum = max(C * e32, esum)
  notes["sum"] = abs(float(got["out4"][0]) - float(ref["sum"])) / bsum if bsum > 0 else float(got["out4"][0] != 0)
  assert notes["sum"] <= 1.0, (tag, "sum", float(got["out4"][0]), float(ref["sum"]), bsum)
  if n == 0:
    # the reference's loss is 0 / 0: NaN; its gradient through autograd is exactly 0 — so must the kernel's be (gs = g_mean /
    # count is inf in the backward pass; nothing of it may reach g_pred)
    assert math.isnan(float(got["out4"][2])) and math.isnan(float(o32["mean"])) and float(got["out4"][0]) == 0.0
    assert bool((got["g_mean"] == 0).all()), "g_mean path: %d non-zero / non-finite" % int((got["g_mean"] != 0).sum())
    assert bool((got["g_sum"] == 0).all())
    assert bool((o32["g_mean"] == 0).all())
    parity_note("photometric_chain[%s]" % tag, **notes)
    return notes
  bmean = max(C * abs(float(o32["mean"]) - float(ref["mean"])), bsum / n + 2 * U * abs(float(ref["mean"])))
  notes["mean"] = abs(float(got["out4"][2]) - float(ref["mean"])) / bmean
  assert notes["mean"] <= 1.0, (tag, "mean", float(got["out4"][2]), float(ref["mean"]), bmean)
  assert float(got["mean"]) == float(got["out4"][2])

  # d loss / d pred: grad_scale sums the magnitudes of the terms the kernel adds (SSIM coefficients with their cancellation,
  # L1, smoothness, the per-image mean term) in units of the result; K = 32: a coefficient passes ~12 roundings, its 3x3 gather
  # 9 more, the warp's slope and multiplier 4.  Plus, only next to the smoothness band (neighbours whose normalised disparities
  # lie within 4 ulp: their sign follows the rounding of the per-image mean, which the kernels sum in fp64 and the oracle in
  # fp32), the most a sign that differs there (0 against +-1) can move the gradient (photometric_ref.smooth_band_allowance).
  notes["smooth_band_edges"] = int(dec["sx_band"].sum() + dec["sy_band"].sum())
  for which, gs in (("g_mean", 1.0 / n), ("g_sum", 1.0)):
    gsc = pr.grad_scale(ref, H, W, gs, dy)
    r64 = ref["g_sum"] * gs
    notes[which] = ratio(got[which], r64, o32[which], gsc, 32, "%s %s" % (tag, which), pr.smooth_band_allowance(ref, dec, gs))
    # the gradient is not trivially zero where the reference's is not
    assert float(got[which].abs().max()) > 0.0 or float(r64.abs().max()) == 0.0
  if band_share_max is not None:
    notes["band_share"] = notes["band"] / float(B * H * W)
    assert notes["band_share"] <= band_share_max, notes
  parity_note("photometric_chain[%s]" % tag, **notes)
  return notes


WORKLOADS = [(4, 375, 1242), (1, 375, 1242), (2, 540, 960)]


@pytest.mark.parametrize("B,H,W", WORKLOADS)
def test_chain_workloads_against_fp64(B, H, W):
  """the bench's shape, batch 1 and a 540 x 960 pair, random images and disparities.  The decision band (exact sample
  coordinate within two ulp of an integer, not on it) is a share of at most 2^-21 * W of the pixels: the band's width,
  2^-21 * |k| around the integer k <= W, over a unit spacing of the integers (5.9e-4 at W = 1242)."""
  check_chain("random %dx%dx%d" % (B, H, W), *make_inputs("random", B, H, W, seed=B + H), band_share_max=2.0 ** -21 * W)


def test_chain_disparities_up_to_W_full_size():
  check_chain("disp_to_W 1x375x1242", *make_inputs("disp_to_W", 1, 375, 1242, seed=5), band_share_max=2.0 ** -21 * 1242)


@pytest.mark.parametrize("B,H,W", [(2, 2, 64), (1, 7, 64), (2, 8, 64), (1, 9, 64), (1, 15, 64), (2, 16, 64), (1, 17, 64),
                                   (1, 9, 2), (1, 9, 59), (2, 9, 60), (1, 9, 61), (1, 9, 62), (1, 9, 119), (1, 9, 120), (2, 9, 121),
                                   (1, 9, 124), (1, 9, 125), (64, 2, 2), (300, 3, 5)])
def test_chain_strip_and_block_edges(B, H, W):
  """heights around the 8-row strips, widths around the 60-column (backward) and 62-column (forward) blocks, and the
  workspace-sizing branch where B * 512 > 2 * units (64 images of 2 x 2, 300 of 3 x 5)"""
  check_chain("edges %dx%dx%d" % (B, H, W), *make_inputs("random", B, H, W, seed=3 * H + W))


FAMILIES = [
  ("ties", 2, 32, 128), ("ties", 1, 64, 256), ("near_identical", 2, 32, 128), ("near_identical", 1, 64, 256),
  ("mask_clip", 2, 16, 64), ("mask_clip", 1, 32, 256), ("mask_clip", 1, 17, 125), ("mask_clip", 1, 40, 1242),
  ("one_valid", 1, 16, 64), ("one_image_invalid", 3, 16, 61), ("all_invalid", 2, 9, 61),
  ("const_pred", 2, 16, 64), ("zero_pred", 1, 16, 64), ("tiny_pred", 2, 16, 125),
]


@pytest.mark.parametrize("family,B,H,W", FAMILIES)
def test_chain_decision_edges(family, B, H, W):
  notes = check_chain("%s %dx%dx%d" % (family, B, H, W), *make_inputs(family, B, H, W, seed=11))
  if family in ("ties", "near_identical"):
    left, right, pred = make_inputs(family, B, H, W, seed=11)
    dec = pr.decisions(left, right, pred)
    # the family reaches what it is for: exact-zero L1 and smoothness differences, and (near_identical) clamped SSIM windows
    assert float((dec["l1_sign"] == 0).float().mean()) > (0.3 if family == "ties" else -1)
    assert float((dec["sx_sign"] == 0).float().mean()) > 0.3
    if family == "near_identical":
      assert float((~dec["ssim_pass"]).float().mean()) > 0.05
  if family == "one_valid":
    assert notes["count"] == 1
  if family == "mask_clip":
    left, right, pred = make_inputs(family, B, H, W, seed=11)
    dec = pr.decisions(left, right, pred)
    assert bool(dec["cx"][dec["mask"]].any()) and bool((~dec["mask"]).any())


# ----------------------------------------------------------------------------------------------------------------------------
# the row kernels' four maps, directly against fp64
# ----------------------------------------------------------------------------------------------------------------------------
def maps_ref(pred, img, warped):
  """fp64 loss maps (the oracle's monodepth_loss in float64: no gradient, no decision but the clamp's values, which are
  continuous) and the parts map_scales needs"""
  from oracle import stereo_oracle as orc
  P, L, Y = pred.double(), img.double(), warped.double()
  total, l1, ssim, smooth = orc.monodepth_loss(P, L, Y, pr.SW)
  raw, mu_x, mu_y, _, _, _, A1, A2, B1, B2, n, d = pr._ssim_parts(L, Y)
  mean_disp = P.mean(2, True).mean(3, True)
  nd = P / (mean_disp + 1e-7)
  ex = torch.exp(-(L[..., :-1] - L[..., 1:]).abs().mean(1, keepdim=True))
  ey = torch.exp(-(L[..., :-1, :] - L[..., 1:, :]).abs().mean(1, keepdim=True))
  ref = dict(total=total, parts=dict(L=L, warped=Y, mu_x=mu_x, mu_y=mu_y, B2=B2, nd=nd, ex=ex, ey=ey))
  o = [t.double() for t in orc.monodepth_loss(pred, img, warped, pr.SW)]
  return dict(total=total, l1=l1, ssim=ssim, smooth=smooth), o, pr.map_scales(ref, *img.shape[-2:])


@pytest.mark.parametrize("family,B,H,W", [("random", 1, 375, 1242), ("random", 2, 9, 61), ("random", 1, 17, 125), ("random", 3, 2, 2),
                                          ("ties", 2, 32, 128), ("near_identical", 1, 64, 256), ("tiny_pred", 1, 16, 64),
                                          ("const_pred", 1, 8, 60)])
def test_monodepth_loss_rows_maps_against_fp64(family, B, H, W):
  """as_monodepth_loss_rows_fwd's total / l1 / ssim / smooth maps on a given warped image.  K per map (roundings on the way):
  l1 4 (three differences, two additions, one division), ssim 16 (the pooled moments' 9 additions and the SSIM formula; the
  cancellation in the scale), smooth 12 (division by the mean, differences, exp, products), total 24 (the three plus their sum)."""
  left, right, pred = make_inputs(family, B, H, W, seed=29)
  warped = pr.orc.linear_warp(right, pred, True)[0]
  lib = nat.load()
  ws = torch.empty(lib.as_photometric_chain_workspace(B, H, W), device=DEV)
  got = [torch.full((B, 1, H, W), float("nan"), device=DEV) for _ in range(4)]
  pd, ld, wd = pred.to(DEV), left.to(DEV), warped.to(DEV)
  nat.call("as_monodepth_loss_rows_fwd", nat.ptr(pd), nat.ptr(ld), nat.ptr(wd), B, H, W, pr.SW, *[nat.ptr(t) for t in got],
           nat.ptr(ws), nat.stream())
  torch.cuda.synchronize()
  ref, o32, sc = maps_ref(pred, left, warped)
  notes = {}
  for i, (name, K) in enumerate((("total", 24), ("l1", 4), ("ssim", 16), ("smooth", 12))):
    notes[name] = ratio(got[i], ref[name], o32[i], sc[name], K, "%s rows %s" % (family, name))
  parity_note("monodepth_rows_maps[%s %dx%dx%d]" % (family, B, H, W), **notes)


def test_rows_entry_points_refuse_a_single_row_or_column():
  """rows_args_ok: H == 1 or W == 1 has no 3x3 stencil of the kind the strips assume; every entry point refuses it with a
  non-zero status (and the workspace query with -1) before anything is launched"""
  lib = nat.load()
  t = torch.zeros(64, device=DEV)
  m = torch.zeros(64, dtype=torch.uint8, device=DEV)
  one = torch.ones(1, device=DEV)
  for (B, H, W) in ((1, 1, 8), (1, 8, 1), (2, 1, 1)):
    assert lib.as_photometric_chain_workspace(B, H, W) == -1
    rc = lib.as_photometric_chain_fwd(nat.ptr(t), nat.ptr(t), nat.ptr(t), B, H, W, pr.SW, nat.ptr(t), nat.ptr(m), nat.ptr(t),
                                      nat.ptr(t), nat.stream())
    assert rc != 0
    rc = lib.as_photometric_chain_bwd(nat.ptr(one), None, nat.ptr(t), nat.ptr(t), nat.ptr(t), nat.ptr(t), B, H, W, pr.SW,
                                      nat.ptr(t), nat.ptr(t), nat.ptr(t), nat.stream())
    assert rc != 0
    rc = lib.as_monodepth_loss_rows_fwd(nat.ptr(t), nat.ptr(t), nat.ptr(t), B, H, W, pr.SW, nat.ptr(t), None, None, None,
                                        nat.ptr(t), nat.stream())
    assert rc != 0
  torch.cuda.synchronize()
  assert float(t.abs().sum()) == 0.0
