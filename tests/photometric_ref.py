"""fp64 reference of the adaptation step's photometric chain (warp right -> left, monodepth loss map, masked mean), with the
reference's own discrete decisions.

This restates ``orc.monodepth_single_loss`` (oracle/stereo_oracle.py: linear_warp, monodepth_loss) with every continuous
quantity in the dtype asked for (float64 for the GPU tests) and its gradient from torch autograd.  Where fp32 and fp64 would
take a different discrete branch, the branch is the one a float32 run of the oracle takes on the same inputs, because that is
the reference's arithmetic:

- the validity mask ``-1 <= nx <= 1`` (from the fp32 ``nx = 2 (x - d) / W - 1``);
- the border clip of the sample coordinate and its zero gradient (``u <= 0`` or ``u >= W - 1``, borders count as clipped);
- the bilinear cell (``floor`` of the fp32 clipped sample coordinate);
- the SSIM clamp's pass map (``0 <= (1 - n/d)/2 <= 1`` in fp32);
- the signs of the L1 and smoothness differences (``sign(0) = 0``, as torch's ``abs`` backward).

The values on those branches are in the requested dtype.  In float32 the module follows torch's CPU rounding, which fuses
the sample coordinate ``(nx + 1) * (W / 2) - 1/2`` and the bilinear sum into fmas (one rounding each, as the kernels'
``fma(nx + 1, W, -1) / 2``), so a float32 run reproduces the oracle's forward bits.  Pixels whose exact sample coordinate lies
within two ulp of an integer without being one form the *decision band*: there fp32 and fp64 take different cells or clips,
and only the pinning keeps the fp64 comparison meaningful.  The band is reported, and asserted to be rare on random inputs.
A second band is the smoothness sign's: neighbours whose normalised disparities lie within 4 ulp.  Their sign follows the
rounding of the per-image mean, which the kernels accumulate in fp64 and the oracle in fp32; ``smooth_band_allowance`` is the
most a flipped sign there can move the gradient.
"""
import torch
import torch.nn.functional as F

from oracle import stereo_oracle as orc

U = 2.0 ** -24           # unit roundoff of binary32
SW = 1e-3                # the adaptation step's smoothness weight (adapt.py:80)


# ----------------------------------------------------------------------------------------------------------------------------
# fp32 oracle, with autograd
# ----------------------------------------------------------------------------------------------------------------------------
def oracle32(left, right, pred):
  """orc.monodepth_single_loss in float32 -> dict(mean, sum, count, warped, mask, total, g_mean, g_sum); g_* = d (mean | sum)
  / d pred for an upstream gradient of 1."""
  p = pred.detach().float().clone().requires_grad_(True)
  warped, mask = orc.linear_warp(right.float(), p, True)
  total = orc.monodepth_loss(p, left.float(), warped, SW)[0]
  sel = total[mask]
  s, m = sel.sum(), sel.mean()
  g_sum, = torch.autograd.grad(s, p, retain_graph=True)
  g_mean, = torch.autograd.grad(m, p)
  return dict(mean=m.detach(), sum=s.detach(), count=int(mask.sum()), warped=warped.detach(), mask=mask, total=total.detach(),
              g_mean=g_mean, g_sum=g_sum)


# ----------------------------------------------------------------------------------------------------------------------------
# the reference's decisions, from a float32 run
# ----------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
  """a * b + c rounded once in a's dtype (float32: the exact product in fp64, then one addition, then to fp32 — the same as
  a fused multiply-add but for a double rounding that needs the fp64 sum to fall exactly half-way, ~2^-29 of the cases)"""
  if a.dtype == torch.float32:
    return (a.double() * b.double() + c.double()).float()
  return a * b + c


def _clip(u, size):
  """border clip of the reference (borders count as clipped) -> (clipped value, clipped?)"""
  hi = float(size - 1)
  lo_c, hi_c = u <= 0, u >= hi
  return torch.where(lo_c, torch.zeros_like(u), torch.where(hi_c, torch.full_like(u, hi), u)), lo_c | hi_c


def _ssim_parts(x, y):
  """the oracle's ssim_distance before the clamp, in x's dtype -> (raw, mu_x, mu_y, sig_x, sig_y, sig_xy, A1, A2, B1, B2, n, d)"""
  c1, c2 = 0.01 ** 2, 0.03 ** 2
  pool = lambda t: F.avg_pool2d(t, 3, stride=1, padding=1)
  mu_x, mu_y = pool(x), pool(y)
  sig_x = pool(x ** 2) - mu_x ** 2
  sig_y = pool(y ** 2) - mu_y ** 2
  sig_xy = pool(x * y) - mu_x * mu_y
  A1, A2 = 2 * mu_x * mu_y + c1, 2 * sig_xy + c2
  B1, B2 = mu_x ** 2 + mu_y ** 2 + c1, sig_x + sig_y + c2
  n, d = A1 * A2, B1 * B2
  return (1 - n / d) / 2, mu_x, mu_y, sig_x, sig_y, sig_xy, A1, A2, B1, B2, n, d


def decisions(left, right, pred):
  """The fp32 oracle's discrete decisions (see the module docstring) and the decision band, all [B,1,H,W] / [B,3,H,W]."""
  left, right, p32 = left.float(), right.float(), pred.detach().float()
  B, _, H, W = right.shape
  xs = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W)
  ys = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1).expand(B, 1, H, W)
  fx = xs - p32                                                     # linear_warp: gx - d, 2 gx / w - 1
  nx = 2 * fx / W - 1.0
  ny = 2 * ys / H - 1.0
  mask = (nx >= -1.0) & (nx <= 1.0) & (ny >= -1.0) & (ny <= 1.0)
  ux = _fma(nx + 1, torch.full_like(nx, W / 2.0), torch.full_like(nx, -0.5))     # grid_sample(align_corners=False) un-normalised
  uy = _fma(ny + 1, torch.full_like(ny, H / 2.0), torch.full_like(ny, -0.5))
  ix, cx = _clip(ux, W)
  iy, cy = _clip(uy, H)
  # band: the exact value a*W/2 - 1/2 (a = nx + 1, an fp32 number; the product is exact in fp64) is not an integer but lies
  # within 2^-22 * max(|k|, 1) of one (two ulp of k): one rounding or two can then leave it on either side of k, or on it
  uxe = (nx.double() + 1) * (W / 2.0) - 0.5
  k = torch.round(uxe)
  band = (uxe != k) & ((uxe - k).abs() <= 2.0 ** -22 * k.abs().clamp(min=1.0))
  warped32, _ = orc.linear_warp(right, p32, True)
  raw32 = _ssim_parts(left, warped32)[0]
  mean32 = p32.mean(2, True).mean(3, True)
  nd32 = p32 / (mean32 + 1e-7)
  # smoothness band: neighbours whose normalised disparities differ by at most 4 ulp (the disparities themselves differ).  The
  # sign of their difference rests on the rounding of the per-image mean, which a kernel may sum in another order or precision
  band4 = lambda a, b: (a - b).abs() <= 2.0 ** -21 * torch.maximum(a.abs(), b.abs())
  sxb = band4(nd32[..., :-1], nd32[..., 1:]) & (p32[..., :-1] != p32[..., 1:])
  syb = band4(nd32[..., :-1, :], nd32[..., 1:, :]) & (p32[..., :-1, :] != p32[..., 1:, :])
  return dict(mask=mask, cx=cx, ixc=ix, cy=cy, iyc=iy, x0=torch.floor(ix).long(), y0=torch.floor(iy).long(),
              band=band, sx_band=sxb, sy_band=syb, ssim_pass=(raw32 >= 0) & (raw32 <= 1), l1_sign=torch.sign(left - warped32),
              sx_sign=torch.sign(nd32[..., :-1] - nd32[..., 1:]), sy_sign=torch.sign(nd32[..., :-1, :] - nd32[..., 1:, :]))


# ----------------------------------------------------------------------------------------------------------------------------
# the chain on those decisions
# ----------------------------------------------------------------------------------------------------------------------------
def _taps(img, x0, y0):
  """the four bilinear taps of the cell (x0, y0) of every pixel, zero beyond the last column / row (grid_sample's
  within_bounds) -> nw, ne, sw, se [B,C,H,W]"""
  B, C, H, W = img.shape
  flat = img.reshape(B, C, H * W)

  def tap(xx, yy):
    ok = (xx <= W - 1) & (yy <= H - 1)
    i = (yy.clamp(max=H - 1) * W + xx.clamp(max=W - 1)).reshape(B, 1, H * W).expand(B, C, H * W)
    return torch.gather(flat, 2, i).reshape(B, C, H, W) * ok.to(img.dtype)
  return tap(x0, y0), tap(x0 + 1, y0), tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)


def _geometry(pred, dec, W, H, dt):
  """sample coordinates on the decided branches: the clipped ones are the clip's constant (no gradient)"""
  xs = torch.arange(W, dtype=dt).view(1, 1, 1, W)
  ys = torch.arange(H, dtype=dt).view(1, 1, H, 1)
  fx = xs - pred
  nx = 2 * fx / W - 1.0
  ny = 2 * ys / H - 1.0
  ux = _fma(nx + 1, torch.full_like(nx, W / 2.0), torch.full_like(nx, -0.5))
  uy = _fma(ny + 1, torch.full_like(ny, H / 2.0), torch.full_like(ny, -0.5))
  ix = torch.where(dec["cx"], dec["ixc"].to(dt), ux)
  iy = torch.where(dec["cy"], dec["iyc"].to(dt), uy.expand_as(ix))
  return fx, ix, iy, dec["x0"], dec["y0"]


def chain(left, right, pred, dec, dt=torch.float64):
  """The oracle's monodepth_single_loss in dtype dt on the fp32 decisions `dec`.  -> dict with
  warped, total, l1, ssim, smooth (maps), sum, mean, count, g_sum = d sum / d pred, g_mean = g_sum / count,
  gw = d sum / d warped, and `parts` (fp64 intermediates the error bounds are built from)."""
  B, C, H, W = right.shape
  L, R = left.to(dt), right.to(dt)
  p = pred.detach().to(dt).clone().requires_grad_(True)
  fx, ix, iy, x0, y0 = _geometry(p, dec, W, H, dt)
  x0f, y0f = x0.to(dt), y0.to(dt)
  w = ix - x0f; e = 1 - w                      # grid_sample: distances to the cell's sides
  n_ = iy - y0f; s = 1 - n_
  nw, ne, sw, se = _taps(R, x0, y0)
  warped = _fma(se, n_ * w, _fma(sw, n_ * e, _fma(ne, s * w, nw * (s * e))))
  warped.retain_grad()

  raw, mu_x, mu_y, sig_x, sig_y, sig_xy, A1, A2, B1, B2, n, d = _ssim_parts(L, warped)
  ssim_c = torch.where(dec["ssim_pass"], raw, raw.clamp(0, 1).detach())
  photo_ssim = ssim_c.mean(dim=1, keepdim=True)
  photo_l1 = (dec["l1_sign"].to(dt) * (L - warped)).mean(dim=1, keepdim=True)
  mean_disp = p.mean(2, True).mean(3, True)
  nd = p / (mean_disp + 1e-7)
  gix = (L[..., :-1] - L[..., 1:]).abs().mean(1, keepdim=True)
  giy = (L[..., :-1, :] - L[..., 1:, :]).abs().mean(1, keepdim=True)
  tx = dec["sx_sign"].to(dt) * (nd[..., :-1] - nd[..., 1:]) * torch.exp(-gix)
  ty = dec["sy_sign"].to(dt) * (nd[..., :-1, :] - nd[..., 1:, :]) * torch.exp(-giy)
  smooth = F.pad(tx, (0, 1)) + F.pad(ty, (0, 0, 0, 1))
  total = 0.85 * photo_ssim + 0.15 * photo_l1 + SW * smooth
  mask = dec["mask"]
  sel = total[mask]
  lsum = sel.sum()
  count = int(mask.sum())
  if count:
    lsum.backward()
    g_sum, gw = p.grad.detach(), warped.grad.detach()
  else:                                         # nothing valid: the sum is a constant 0, its gradient exactly 0
    g_sum, gw = torch.zeros_like(p), torch.zeros_like(warped)
  dix = (ne - nw) * s + (se - sw) * n_          # d warped / d ix on the decided cell
  parts = dict(fx=fx.detach(), dix=dix.detach(), taps=(nw.detach(), ne.detach(), sw.detach(), se.detach()), w=w.detach(),
               n=n_.detach(), mu_x=mu_x.detach(), mu_y=mu_y.detach(), B1=B1.detach(), B2=B2.detach(), A1=A1.detach(),
               A2=A2.detach(), nn=n.detach(), d=d.detach(), nd=nd.detach(), mean_disp=mean_disp.detach(), ex=torch.exp(-gix).detach(),
               ey=torch.exp(-giy).detach(), L=L, warped=warped.detach())
  return dict(mask=mask, warped=warped.detach(), total=total.detach(), l1=photo_l1.detach(), ssim=photo_ssim.detach(), smooth=smooth.detach(),
              sum=lsum.detach(), count=count, mean=(lsum / count).detach() if count else lsum.detach() / 0.0,
              g_sum=g_sum, g_mean=g_sum / count if count else g_sum.clone(), gw=gw, parts=parts)


# ----------------------------------------------------------------------------------------------------------------------------
# error scales: the magnitudes the fp32 arithmetic rounds, per element (see the bounds in tests/test_gpu_photometric_chain.py)
# ----------------------------------------------------------------------------------------------------------------------------
def _pool(t):
  return F.avg_pool2d(t, 3, stride=1, padding=1)


def _ssim_mag(x, y, mu_x, mu_y, B2):
  """M = E[x^2] + mu_x^2 + E[y^2] + mu_y^2 + 2 (E|xy| + |mu_x mu_y|): what the sigma terms cancel; an fp32 evaluation's
  absolute error in sig_x + sig_y + 2 |sig_xy| is a few u * M.  Returned over B2 (>= |A2| and >= C2 > 0)."""
  M = _pool(x * x) + mu_x ** 2 + _pool(y * y) + mu_y ** 2 + 2 * (_pool((x * y).abs()) + (mu_x * mu_y).abs())
  return M / B2


def warp_scale(ref, H, W):
  """per-element scale of the fp32 warped image: the taps it sums, plus the slope times the sample coordinate's rounding
  (x - d, 2 fx / W, - 1, + 1, * W/2, - 1/2: each rounds at most u * (|fx| + 2W + 1) in units of ix)"""
  P = ref["parts"]
  nw, ne, sw, se = P["taps"]
  w, n_ = P["w"], P["n"]
  vals = nw.abs() * ((1 - n_) * (1 - w)).abs() + ne.abs() * ((1 - n_) * w).abs() + sw.abs() * (n_ * (1 - w)).abs() + \
      se.abs() * (n_ * w).abs()
  coord = P["fx"].abs() + 2 * W + 1
  # the y coordinate (2y/H - 1, + 1, * H/2, - 1/2) rounds up to u * (3H + 1): slope (sw - nw), (se - ne)
  dy = ((sw - nw).abs() + (se - ne).abs()) * (3 * H + 1)
  return vals + P["dix"].abs() * coord + dy


def map_scales(ref, H, W, wscale=None):
  """per-pixel scales of the four loss maps [B,1,H,W]: l1, ssim, smooth, total.  wscale = the warped image's own error scale
  (in units of u) when the warped image is computed, None when it is given."""
  P = ref["parts"]
  L, Y = P["L"], P["warped"]
  dy = wscale if wscale is not None else torch.zeros_like(Y)
  l1 = ((L - Y).abs() + L.abs() + Y.abs() + dy).mean(1, keepdim=True)
  rel = _ssim_mag(L, Y, P["mu_x"], P["mu_y"], P["B2"])
  # raw = (1 - n/d)/2: n/d carries ~ u * (1 + M/B2) relatively (|n/d| <= 1 here or clamped); an input error dy moves the
  # pooled moments by ~ (2|y| + |x| + 2) * dy / B2 relatively
  dmom = _pool(dy * (2 * Y.abs() + L.abs() + 2)) / P["B2"]
  ssim = (1 + rel + dmom).mean(1, keepdim=True)
  nd = P["nd"]
  ex, ey = P["ex"], P["ey"]
  sx = F.pad(ex * (nd[..., :-1].abs() + nd[..., 1:].abs() + (nd[..., :-1] - nd[..., 1:]).abs()), (0, 1))
  sy = F.pad(ey * (nd[..., :-1, :].abs() + nd[..., 1:, :].abs() + (nd[..., :-1, :] - nd[..., 1:, :]).abs()), (0, 0, 0, 1))
  smooth = sx + sy
  total = 0.85 * ssim + 0.15 * l1 + SW * smooth + ref["total"].abs()
  return dict(l1=l1, ssim=ssim, smooth=smooth, total=total)


def grad_scale(ref, H, W, gs, wscale):
  """per-pixel scale of d (gs * sum) / d pred [B,1,H,W] (gs: the loss map's gradient at a valid pixel, 0 elsewhere).
  Built from the terms the kernel's fp32 sums add: the SSIM coefficients a, b, c of each window (with the cancellation of
  their A2 - A1, B2 - B1 and n/d: relative M/B2, plus the moments' shift by the warped image's own error), the L1 term,
  the slope, the smoothness terms and the per-image mean term."""
  P = ref["parts"]
  L, Y = P["L"], P["warped"]
  mu_x, mu_y, A1, A2, B1, B2, n, d = (P[k] for k in ("mu_x", "mu_y", "A1", "A2", "B1", "B2", "nn", "d"))
  g = gs * ref["mask"].to(L.dtype)
  Gq = (0.85 / 3 * 0.5) * g
  rel = _ssim_mag(L, Y, mu_x, mu_y, B2)
  dmom = _pool(wscale * (2 * Y.abs() + L.abs() + 2)) / B2
  r = 1 + rel + dmom
  a_m = Gq * (2 * mu_x.abs() * (A2.abs() + A1.abs()) * d + n.abs() * 2 * mu_y.abs() * (B2 + B1)) / d ** 2 * r
  b_m = Gq * (n * B1).abs() / d ** 2 * r
  c_m = Gq * 2 * A1.abs() / d * r
  gw_m = _pool(a_m + 2 * b_m * Y.abs() + c_m * L.abs()) + 2 * _pool(b_m) * wscale + 0.05 * g
  nw, ne, sw, se = P["taps"]
  dix_m = P["dix"].abs() + ((ne - nw).abs() + (se - sw).abs()) * (3 * H + 1) * U     # (the y weights' rounding, times u)
  warp = (gw_m * dix_m).sum(1, keepdim=True)
  nd = P["nd"]
  ex, ey = P["ex"], P["ey"]
  den = P["mean_disp"] + 1e-7
  s_m = torch.zeros_like(nd)
  s_m[..., :-1] += ex
  s_m[..., 1:] += ex
  s_m[..., :-1, :] += ey
  s_m[..., 1:, :] += ey
  s_m = SW * abs(gs) * s_m / den                         # |g_direct| = |sum of up to four sw * gt * w * sign| / den
  mean_term = (s_m * nd.abs()).sum((1, 2, 3), keepdim=True) / (H * W)      # S_b / den^2 / plane = sum g_direct * nd / plane
  return warp + s_m + mean_term


def smooth_band_allowance(ref, dec, gs):
  """what the smoothness band's signs can move d (gs * sum) / d pred by [B,1,H,W].
  An edge (a, b) of the band adds y * sign(nd_a - nd_b) to g_nd at a and its negative at b, y = sw * gt_a * w.  For one den,
  fp32 division is monotone (increasing for den > 0, decreasing for den < 0), and the kernel's den and the oracle's are two
  roundings of the same mean: both order nd_a, nd_b as pred_a, pred_b, or one of them rounds them equal.  So the two signs
  differ at most as 0 against +-1: one y.  That moves g_direct = g_nd / den at a and at b by y / |den|, and the per-image
  mean term sum(g_direct * nd) / plane at every pixel of the image by y |nd_a - nd_b| / (|den| plane)."""
  P = ref["parts"]
  g = gs * ref["mask"].to(P["nd"].dtype)
  den = (P["mean_disp"] + 1e-7).abs()
  nd = P["nd"]
  ex = SW * g[..., :-1] * P["ex"] * dec["sx_band"].to(nd.dtype) / den
  ey = SW * g[..., :-1, :] * P["ey"] * dec["sy_band"].to(nd.dtype) / den
  out = torch.zeros_like(nd)
  out[..., :-1] += ex
  out[..., 1:] += ex
  out[..., :-1, :] += ey
  out[..., 1:, :] += ey
  mean = ((ex * (nd[..., :-1] - nd[..., 1:]).abs()).sum((1, 2, 3), keepdim=True) +
          (ey * (nd[..., :-1, :] - nd[..., 1:, :]).abs()).sum((1, 2, 3), keepdim=True)) / nd[0].numel()
  return out + mean
