"""A plain float64 restatement of ONE launch each of the two ends of the cost-aggregation chain: the difference cost volume and
its adjoint (csrc/cost_volume.hip), the fused tail as_agg_tail_fwd (csrc/agg_tail.hip: the 32 -> 1 3-D convolution to logits,
soft-argmax, arg-max, feature-contrast score), its one-launch backward as_agg_tail_bwd (csrc/agg_tail_bwd.hip) and the
first-generation launches of csrc/softargmax.hip (as_conv3d_out_fwd / _bwd, as_softargmax_fwd / _bwd), the bound of every output,
and the cases the GPU file (tests/test_gpu_tail_fp64.py) runs.  CPU only: nothing here imports the library.
tests/test_tail_ref_cpu.py holds the restatements to torch's float64 autograd, brackets a float32 emulation of each loop with
the bounds and shows that the cases tell deliberately wrong restatements (MUTANTS) from the right one.

Tensors are channel-last: volumes are [B, D, H, W, 32] (a PCL interior), the weights are conv3d_alone.weight[0], [32][3][3][3],
tap t = 9 kd + 3 kh + kw; logits are [B, D, H, W], maps [B, H, W]; feature maps of the cost volume are torch's [B, 32, H, W].

Bounds follow trunk_ref's rule, derived and never tuned: a sum of n fp32 terms added in ANY order errs by at most
gamma(n) sum|terms|; elementwise steps count their roundings, first order, in U = 2^-24.
  cost volume      forward: one subtract, the correctly rounded difference (bit-exact).  Backward: gL[x] has min(x, D - 1) + 1
                   terms, gR[x] as many as there are d with x + d < W: gamma(n) sum|g|.
  logits           bias + conv3d(a, w): n = 32 * 27 + 1, gamma(n) (conv(|a|, |w|) + |bias|).  With the input BatchNorm the
                   operand is a = lrelu(fma(x, scale, shift)): trunk_ref's K_OP treatment, e_a = K_OP U (|x scale| + |shift|)
                   per voxel (the by-product a_out is held to it directly), which reaches the logits through conv(e_a, |w|).
  soft-argmax      from the kernel's OWN fp32 logits l (widened): with x_d = l_d - m, p the soft-max, K_EXP the error of the
                   device's expf in ulps,
                     eps_d  = (|x_d| + 2 K_EXP) U          the rounded subtraction, magnified by exp, and expf itself
                     eps_se = sum_d p_d eps_d + gamma(D)    the sum of the exponentials
                     e_pred = sum_d d p_d (eps_d + eps_se + 2 U) + gamma(D) pred     (the quotient and the product: 2 U)
  FCS              m1 - (sum - m1 - m2) / (D - 2), linear in the logits:
                     e_fcs = gamma(D + 2) (sum|l| + |m1| + |m2|) / (D - 2) + U |m1| + 2 U |fcs|;   0 for D <= 2 (fcs = 0)
  arg-max          the first maximum of the kernel's own logits, everywhere; the reference's wherever the reference's top-2 gap
                   exceeds 2 max_d e_logit (elsewhere the pixel is undecided: UNDECIDED_CAP of the pixels at most)
  tail backward    g_logits = p_d (d - pred) g_pred + g_in from the same pieces: p_d errs by eps_p = eps_d + eps_se + U
                   (relative), pred by e_pred, d - pred rounds once, the two products once each, the add once:
                     e_gl = |g_pred| p_d (|d - pred| (eps_p + 3 U) + e_pred) + U |g_logits|     (0 without g_pred: a copy)
                   g_a = conv_transpose(g_logits, w), n = 27: gamma(27) convT(|g_logits|, |w|) + convT(e_gl, |w|)
                   g_w, g_bias: n = B D H W (+ 1 with accumulate: the value already there joins the sum):
                     gamma(n) (sum |a| |g_logits| (+ |prior|)) + sum |a| e_gl,     gamma(n) (sum |g_logits| (+ |prior|)) + sum e_gl
                   the slab split and the fp64 slab reduction do not enter: the rule holds for any order.

Underflow.  The relative model ends at the smallest normal number TINY = 2^-126: an exponential below it (x_d < -87.3, a
saturated soft-max) comes out denormal or zero, wrong by at most TINY in absolute terms, and so do the quotient p_d (se >= 1)
and the product d p_d: e_pred gains sum_d (2 d + 1) TINY <= D^2 TINY.  In the backward p_d is off by 2 TINY, which reaches
g_logits through |d - pred| |g_pred|, and each of the two products can underflow once more:
e_gl gains TINY (|g_pred| (2 |d - pred| + 1) + 1).  (1e-37: it matters only where the reference itself is below 1e-38.)

K_EXP is the one number that cannot be derived.  It is not fitted to the kernels: 1 ulp for a library expf and the same again
as margin.  tests/test_tail_ref_cpu.py shows the margin on the reference alone (torch's fp32 exp stays inside)."""
import math

import torch
import torch.nn.functional as F

import bn_ref as br
from trunk_ref import U, gamma_n, K_OP, SLOPE    # noqa: F401

TINY = 2.0 ** -126        # the smallest normal fp32 number: what a result below it (flushed or denormal) errs by at most
K_EXP = 2                 # ulps of the device's expf: 1 for a library expf + 1 of margin (not fitted)
UNDECIDED_CAP = 0.01      # share of pixels whose reference arg-max may be left undecided
GAINS = [1.0, 50.0, 300.0]
TAPS = [(kd, kh, kw) for kd in range(3) for kh in range(3) for kw in range(3)]
NAN = float("nan")
F64 = torch.float64


def ratio(got, ref, bound):
  """worst |got - ref| / bound; a NaN in got (never written, or a guard value consumed) counts as infinite"""
  got, ref = got.double().reshape(ref.shape), ref.double()
  if bool(torch.isnan(got).any()):
    return float("inf")
  return br.worst_ratio((got - ref).abs(), bound.double().reshape(ref.shape))


# ----------------------------------------------------------------------------- the dispatch arithmetic
def fwd_npos(H, W):
  """positions of the flattened padded plane from the first interior voxel to the last: (H - 1) Wp + W"""
  return (H - 1) * (W + 2) + W


def fwd_route(geom):
  """positions per workgroup of as_agg_tail_fwd: 0 where as_agg_tail_ok refuses (D > 32, fewer than 32 positions, a run of
  34 + 2 Wp voxels beyond 12 chunks of 32: W > 173), 16 while B ceil(npos / 32) < 512, else 32"""
  B, D, H, W = geom
  n = fwd_npos(H, W)
  if D > 32 or n < 32 or 34 + 2 * (W + 2) > 12 * 32:
    return 0
  return 16 if B * ((n + 31) // 32) < 512 else 32


def fwd_grid(geom):
  B, D, H, W = geom
  return B * ((fwd_npos(H, W) + fwd_route(geom) - 1) // fwd_route(geom))


def bwd_route(geom):
  """columns per unit of as_agg_tail_bwd: 13 while B H ceil(W / 26) <= 768, else 26"""
  B, D, H, W = geom
  return 26 if B * H * ((W + 25) // 26) > 768 else 13


def bwd_units(geom):
  B, D, H, W = geom
  xc = bwd_route(geom)
  return B * H * ((W + xc - 1) // xc)


BWD_GROUPS = 768          # workgroups at most: from there on a workgroup walks several units


# ----------------------------------------------------------------------------- cost volume
def cost_volume(L, R, D):
  """vol[b, d, y, x, c] = fp32(L[b, c, y, x] - R[b, c, y, x - d]) for x >= d, else 0"""
  B, C, H, W = L.shape
  vol = torch.zeros(B, D, H, W, C)
  Lc, Rc = L.double().permute(0, 2, 3, 1), R.double().permute(0, 2, 3, 1)
  for d in range(min(D, W)):
    vol[:, d, :, d:] = (Lc[:, :, d:] - Rc[:, :, :W - d]).float()
  return vol


def _cv_sums(g, dtype):
  B, D, H, W, C = g.shape
  gd = g.to(dtype)
  gL, gR = torch.zeros(B, H, W, C, dtype=dtype), torch.zeros(B, H, W, C, dtype=dtype)
  for d in range(min(D, W)):
    gL[:, :, d:] = gL[:, :, d:] + gd[:, d, :, d:]
    gR[:, :, :W - d] = gR[:, :, :W - d] - gd[:, d, :, d:]
  return gL.permute(0, 3, 1, 2), gR.permute(0, 3, 1, 2)


def cost_volume_bwd(g, dtype=F64):
  """gL[b, c, y, x] = sum_{d <= x} g[b, d, y, x, c],  gR[b, c, y, x'] = - sum_{d, x' + d < W} g[b, d, y, x' + d, c]  (d in
  ascending order) and (float64) their bounds gamma(n) sum|g|, n the number of terms of the pixel's column: min(x, D - 1) + 1
  for gL, min(W - x, D) for gR"""
  B, D, H, W, C = g.shape
  gL, gR = _cv_sums(g, dtype)
  out = dict(gL=gL, gR=gR)
  if dtype == F64:
    x = torch.arange(W)
    nL = (torch.clamp(x, max=D - 1) + 1).double()
    nR = torch.clamp(W - x, max=D).double()
    aL, aR = _cv_sums(g.abs(), F64)
    out.update(nL=nL, nR=nR, e_gL=(nL * U / (1.0 - nL * U)).reshape(1, 1, 1, W) * aL,
               e_gR=(nR * U / (1.0 - nR * U)).reshape(1, 1, 1, W) * -aR)
  return out


# ----------------------------------------------------------------------------- logits
def operand(x, scale=None, shift=None, slope=SLOPE):
  """the convolution's operand and its per-voxel bound: x itself (already activated), or a = lrelu(fma(x, scale, shift)) with
  e_a = K_OP U (|x scale| + |shift|) (the fused multiply-add rounds once, so the branch is the exact sign)"""
  x = x.double()
  if scale is None:
    return x, torch.zeros_like(x)
  sc, sh = scale.double(), shift.double()
  y = x * sc + sh
  return torch.where(y > 0, y, y * slope), K_OP * U * ((x * sc).abs() + sh.abs())


def logits_sum(a, w, bias=None, dtype=F64, mut=None):
  """logits[b, d, y, x] = bias + sum_{kd, kh, kw, c} a[b, d + kd - 1, y + kh - 1, x + kw - 1, c] w[c, kd, kh, kw], a zero outside the
  volume — "project, then shift" as the kernel: every voxel is projected once onto the 27 taps, the taps are added in TAPS order.
  mut:  ("row_off", t)         tap t's offset is one row down
        ("no_shift_back", n)   tiles of n positions, the last one not shifted back to end at npos: its pixels are not written
        ("skip_zero_plane", 1) the pass over the zero plane D + 1, which completes the last logit with its kd = 2 term, is
                               skipped: logit D - 1 is never stored.  (Dropping the term alone changes no value: the plane is zero.)"""
  B, D, H, W, _ = a.shape
  kind, arg = mut if mut is not None else (None, None)
  P = a.to(dtype) @ w.to(dtype).reshape(32, 27)
  Pp = F.pad(P, (0, 0, 1, 1, 1, 2, 1, 1))
  out = torch.zeros(B, D, H, W, dtype=dtype)
  if bias is not None:
    out = out + bias.to(dtype).reshape(())
  for t, (kd, kh, kw) in enumerate(TAPS):
    if not bool(w[:, kd, kh, kw].any()):                     # (a single-tap case: the other taps add exact zeros)
      continue
    dy = kh + (1 if kind == "row_off" and arg == t else 0)
    out = out + Pp[:, kd:kd + D, dy:dy + H, kw:kw + W, t]
  if kind == "no_shift_back":
    pos = torch.arange(H)[:, None] * (W + 2) + torch.arange(W)[None, :]
    out[:, :, pos >= (fwd_npos(H, W) // arg) * arg] = NAN
  if kind == "skip_zero_plane":
    out[:, D - 1] = NAN
  return out


def forward(x, w, bias=None, scale=None, shift=None):
  """a, logits and their bounds:  e_logits = gamma(865) (conv(|a|, |w|) + |bias|) + conv(e_a, |w|)"""
  a, e_a = operand(x, scale, shift)
  aw = w.double().abs()
  e = gamma_n(32 * 27 + 1) * logits_sum(a.abs(), aw, bias.abs() if bias is not None else None)
  if scale is not None:
    e = e + logits_sum(e_a, aw)
  return dict(a=a, e_a=e_a, logits=logits_sum(a, w, bias), e_logits=e)


# ----------------------------------------------------------------------------- soft-argmax, arg-max, FCS
def soft_sum(l, dtype=F64, mut=None):
  """pred = sum_d d softmax(l)_d (the maximum subtracted, sums in d order), the first arg-max, and
  fcs = m1 - (sum - m1 - m2) / (D - 2) with (m1, m2) the two largest as in a sort (0 for D <= 2).
  mut:  "lane_k3"     the lane layout d = j + 8 k breaks beyond k = 2: the disparities from 24 on are left out
        "last_tie"    the last maximum wins a tie
        "fcs_no_dup"  the second value of the FCS must be below the maximum: a duplicate of the maximum is dropped
        "no_max"      the exponentials are taken without subtracting the maximum"""
  l = l.to(dtype)
  B, D, H, W = l.shape
  lv = l[:, :24] if mut == "lane_k3" else l
  Dv = lv.shape[1]
  m1 = lv.max(1)[0]
  e = torch.exp(lv - (torch.zeros_like(m1) if mut == "no_max" else m1)[:, None])
  se = torch.zeros_like(m1)
  for d in range(Dv):
    se = se + e[:, d]
  pred, tot = torch.zeros_like(m1), torch.zeros_like(m1)
  for d in range(Dv):
    pred = pred + (e[:, d] / se) * float(d)
    tot = tot + lv[:, d]
  am = torch.argmax(lv, 1)
  if mut == "last_tie":
    am = Dv - 1 - torch.argmax(lv.flip(1), 1)
  if Dv > 2:
    srt = torch.sort(lv, 1, descending=True)[0]
    m2 = srt[:, 1]
    if mut == "fcs_no_dup":
      below = torch.where(lv < m1[:, None], lv, torch.full_like(lv, -math.inf)).max(1)[0]
      m2 = torch.where(torch.isfinite(below), below, m1)
    fcs = m1 - (tot - m1 - m2) / float(Dv - 2)
  else:
    m2, fcs = m1, torch.zeros_like(m1)
  return dict(pred=pred, argmax=am, fcs=fcs, m1=m1, m2=m2, p=e / se[:, None])


def soft_stage(l):
  """soft_sum of the fp32 logits l, widened, and the bounds of pred and fcs (see the module docstring); eps_p and e_pred also
  serve the backward"""
  l = l.double()
  B, D, H, W = l.shape
  r = soft_sum(l)
  p = r["p"]
  dd = torch.arange(D, dtype=F64).reshape(1, D, 1, 1)
  eps_d = ((l - r["m1"][:, None]).abs() + 2.0 * K_EXP) * U
  eps_se = (p * eps_d).sum(1) + gamma_n(D)
  r["eps_p"] = eps_d + eps_se[:, None] + U
  r["e_pred"] = (dd * p * (eps_d + eps_se[:, None] + 2.0 * U)).sum(1) + gamma_n(D) * r["pred"] + float(D * D) * TINY
  if D > 2:
    r["e_fcs"] = gamma_n(D + 2) * (l.abs().sum(1) + r["m1"].abs() + r["m2"].abs()) / (D - 2) + U * r["m1"].abs() + \
        2.0 * U * r["fcs"].abs()
  else:
    r["e_fcs"] = torch.zeros_like(r["fcs"])
  return r


def decided(logits_ref, e_logits):
  """[B, H, W]: the reference's arg-max is decided — its top-2 gap exceeds 2 max_d e_logit (always, with one disparity)"""
  if logits_ref.shape[1] == 1:
    return torch.ones_like(logits_ref[:, 0], dtype=torch.bool)
  srt = torch.sort(logits_ref.double(), 1, descending=True)[0]
  return (srt[:, 0] - srt[:, 1]) > 2.0 * e_logits.max(1)[0]


# ----------------------------------------------------------------------------- the tail's backward
def logits_gradient(logits, g_pred=None, g_in=None, dtype=F64):
  """g_logits = p_d (d - pred) g_pred + g_in (each may be None: zero) from the fp32 logits the forward saved, and its bound"""
  l = logits.to(dtype)
  B, D, H, W = l.shape
  dd = torch.arange(D, dtype=dtype).reshape(1, D, 1, 1)
  if g_pred is None:
    gl = g_in.to(dtype) if g_in is not None else torch.zeros_like(l)
    return gl, torch.zeros_like(gl, dtype=F64)
  if dtype == F64:
    s = soft_stage(l)
    p, pred = s["p"], s["pred"]
  else:
    s = soft_sum(l, dtype)
    p, pred = s["p"], s["pred"]
  gp = g_pred.to(dtype)[:, None]
  gl = p * (dd - pred[:, None]) * gp
  if g_in is not None:
    gl = gl + g_in.to(dtype)
  if dtype != F64:
    return gl, None
  e = gp.abs() * p * ((dd - pred[:, None]).abs() * (s["eps_p"] + 3.0 * U) + s["e_pred"][:, None]) + \
      TINY * (gp.abs() * (2.0 * (dd - pred[:, None]).abs() + 1.0) + 1.0)
  if g_in is not None:
    e = e + U * gl.abs()
  return gl, e


def tap_stack(gl, mut=None, xc=13):
  """[B, D, H, W, 27]: G_t[v] = g_logits[v - off_t], zero outside the volume (tap t of the forward reaches v from there).
  mut:  ("col_zero", 1)        the staged column x0 - 1 of a chunk of xc columns is taken as zero
        ("plane_rep", "lo"/"hi")  plane -1 (plane D) of the gradient window holds plane 0 (plane D - 1) instead of zero"""
  B, D, H, W = gl.shape
  kind, arg = mut if mut is not None else (None, None)
  gp = F.pad(gl, (1, 1, 1, 1, 1, 1))
  if kind == "plane_rep":
    if arg == "lo":
      gp[:, 0] = gp[:, 1]
    else:
      gp[:, D + 1] = gp[:, D]
  G = torch.stack([gp[:, 2 - kd:2 - kd + D, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W] for (kd, kh, kw) in TAPS], -1)
  if kind == "col_zero":
    first = (torch.arange(W) % xc == 0) & (torch.arange(W) > 0)
    kw2 = torch.tensor([kw == 2 for (_, _, kw) in TAPS])
    G = torch.where(first.reshape(1, 1, 1, W, 1) & kw2.reshape(1, 1, 1, 1, 27), torch.zeros_like(G), G)
  return G


def tail_backward(logits, a, w, g_pred=None, g_in=None, gw0=None, gb0=None, dtype=F64, mut=None, xc=13, groups=BWD_GROUPS):
  """g_a = conv_transpose(g_logits, w), g_w[c, t] = sum_u a[u, c] g_logits[u - off_t] (+ gw0), g_bias = sum g_logits (+ gb0), and
  (float64, no mutant) the bound of each.
  mut:  tap_stack's, or ("skip_second_unit", 1): a unit (image, row, chunk of xc columns) from `groups` on — the second unit of
        a workgroup — is skipped: its g_a is not written, its voxels are missing from g_w and g_bias"""
  B, D, H, W = logits.shape
  kind, arg = mut if mut is not None else (None, None)
  gl, e_gl = logits_gradient(logits, g_pred, g_in, dtype)
  G = tap_stack(gl, mut, xc)
  w27 = w.to(dtype).reshape(32, 27)
  ad = a.to(dtype)
  g_a = G @ w27.t()
  live = torch.ones(B, 1, H, W, dtype=torch.bool)
  if kind == "skip_second_unit":
    nxc = (W + xc - 1) // xc
    unit = (torch.arange(B).reshape(B, 1, 1) * H + torch.arange(H).reshape(1, H, 1)) * nxc + (torch.arange(W) // xc).reshape(1, 1, W)
    live = (unit < groups).reshape(B, 1, H, W)
    g_a = torch.where(live[..., None], g_a, torch.full_like(g_a, NAN))
  lv = live.to(dtype)[..., None]
  g_w = torch.einsum("bdhwc,bdhwt->ct", ad * lv, G)
  g_b = (gl * live.to(dtype)).sum()
  out = dict(gl=gl, e_gl=e_gl)
  if gw0 is not None:
    g_w, g_b = g_w + gw0.to(dtype).reshape(32, 27), g_b + gb0.to(dtype).reshape(())
  out.update(g_a=g_a, g_w=g_w.reshape(32, 3, 3, 3), g_b=g_b.reshape(1))
  if dtype == F64 and mut is None:
    n = B * D * H * W + (1 if gw0 is not None else 0)
    aG, eG, aw = tap_stack(gl.abs()), tap_stack(e_gl), w27.abs()
    out["e_g_a"] = gamma_n(27) * (aG @ aw.t()) + eG @ aw.t()
    s_w = torch.einsum("bdhwc,bdhwt->ct", ad.abs(), aG)
    s_b = gl.abs().sum()
    if gw0 is not None:
      s_w, s_b = s_w + gw0.double().abs().reshape(32, 27), s_b + gb0.double().abs().reshape(())
    out["e_g_w"] = (gamma_n(n) * s_w + torch.einsum("bdhwc,bdhwt->ct", ad.abs(), eG)).reshape(32, 3, 3, 3)
    out["e_g_b"] = (gamma_n(n) * s_b + e_gl.sum()).reshape(1)
  return out


# ----------------------------------------------------------------------------- the geometries the GPU file runs
# as_agg_tail_fwd: (B, D, H, W) and the positions per workgroup.  npos = (H - 1)(W + 2) + W; 16 while B ceil(npos / 32) < 512.
FWD_GEOMS = [
  ((1, 1, 1, 32), 16),      # npos 32: one tile of 32, two of 16; grid 2 (below 8); D = 1
  ((1, 2, 2, 31), 16),      # npos 64; D = 2: one exponential, fcs = 0
  ((3, 3, 2, 17), 16),      # npos 36: three tiles, the last shifted back by 12; grid 9 (not a multiple of 8)
  ((1, 8, 5, 9), 16),       # D = 8: the lane stride of d = j + 8 k, k = 0 only
  ((1, 9, 5, 9), 16),       # D = 9: one lane with k = 1; npos 53, the last tile shifted back by 11
  ((2, 32, 3, 17), 16),     # D = 32: every lane with k = 0 .. 3
  ((1, 12, 3, 173), 16),    # W = 173: the widest run as_agg_tail_ok accepts (34 + 2 * 175 = 384)
  ((8, 12, 24, 78), 16),    # 8 * 60 = 480, below the threshold at the step's own plane
  ((511, 3, 1, 32), 16),    # 511 * 1, just below
  ((512, 3, 1, 32), 32),    # 512 exactly, one tile per image
  ((171, 5, 2, 40), 32),    # npos 82: 171 * 3 = 513 (1 mod 8), the last tile shifted back by 14
  ((9, 12, 24, 78), 32),    # 9 * 60 = 540: the benchmark's batch16 leg from 9 pairs on
  ((13, 4, 8, 156), 32),    # npos 1262: 13 * 40 = 520, Wp = 158
]
FWD_REFUSED = [(1, 3, 2, 174), (1, 33, 3, 17), (1, 3, 1, 31)]     # W = 174, D = 33, npos = 31
# one geometry per route for the flavours that run once per route; the geometries of the exact families
FWD_ONCE = {(3, 3, 2, 17), (171, 5, 2, 40)}
FWD_TAP_GEOMS = [(1, 1, 1, 32), (3, 3, 2, 17), (512, 3, 1, 32), (171, 5, 2, 40)]
FWD_DESIGNED_GEOMS = [(1, 9, 5, 9), (2, 32, 3, 17), (171, 5, 2, 40), (9, 12, 24, 78)]
# as_agg_tail_bwd: (B, D, H, W) and the columns per unit: 13 while B H ceil(W / 26) <= 768
BWD_GEOMS = [
  ((1, 3, 1, 1), 13),       # W = 1
  ((1, 1, 2, 5), 13),       # D = 1
  ((2, 2, 3, 13), 13),      # one full chunk
  ((1, 12, 4, 14), 13),     # a second chunk of one column
  ((2, 32, 3, 27), 13),     # D = 32; chunks of 13, 13 and 1
  ((32, 3, 24, 26), 13),    # 32 * 24 * 1 = 768 exactly; 1536 units of 13 columns: two per workgroup
  ((32, 3, 24, 27), 26),    # 32 * 24 * 2 = 1536 units: a chunk of one column, two units per workgroup
  ((1, 3, 769, 3), 26),     # 769 units, W < 26: workgroup 0 alone takes a second unit
  ((11, 12, 24, 78), 26),   # 11 * 24 * 3 = 792: the benchmark's geometry from 11 pairs on
]
BWD_EXACT_GEOMS = [(1, 3, 1, 1), (2, 2, 3, 13), (1, 12, 4, 14), (1, 3, 769, 3), (32, 3, 24, 26), (32, 3, 24, 27)]
BWD_FIRST_GEN_GEOMS = [(1, 3, 1, 1), (1, 3, 769, 3), (9, 12, 24, 78)]     # (the last: 4096 blocks and 512 slabs, the caps)
CV_GEOMS = [(1, 64, 2, 17), (2, 12, 3, 16), (1, 24, 3, 31), (1, 1, 1, 1)]   # D = 64 > W; W = 16 exactly; W % 16 == 15; smallest


def geom_id(g):
  return "%dx%dx%dx%d" % tuple(g)


# ----------------------------------------------------------------------------- the cases
def _gen(seed):
  return torch.Generator().manual_seed(seed)


# Geometries whose first draw leaves a pixel's arg-max undecided (a plane of 45 or 102 pixels: ONE pixel is beyond the 1 % cap):
# the draw is moved on.  Chosen on the reference alone (tests/test_tail_ref_cpu.py's share test), before any kernel ran.
FWD_SALT = {(1, 9, 5, 9): 2, (2, 32, 3, 17): 1}


def _seed(geom, k):
  B, D, H, W = geom
  return 100003 * k + 7 * B + 1009 * D + 131 * H + W + 1000003 * FWD_SALT.get(tuple(geom), 0)


def chan_scale():
  """different magnitudes per channel, so that a channel swizzle fails"""
  return torch.pow(2.0, (torch.arange(32) % 5 - 2).float())


def add_sentinels(t):
  """+-1e4 in one channel each on the first and the last plane, row and column of the first and the last image: a value that
  reaches an output it does not belong to moves it orders beyond the bound"""
  B, D, H, W, C = t.shape
  spots = [(0, 0, 0), (D - 1, H - 1, W - 1), (0, H - 1, W // 2), (D - 1, 0, W // 2), (D // 2, 0, 0), (D // 2, H - 1, W - 1),
           (0, H // 2, W - 1), (D - 1, H // 2, 0)]
  for bi in sorted({0, B - 1}):
    for k, (d, y, x) in enumerate(spots):
      t[bi, d, y, x, (5 * k + 3 * bi) % C] = 1e4 * (-1.0) ** (k + bi)
  return t


def random_weights(seed, gain=1.0):
  w = torch.randn(32, 3, 3, 3, generator=_gen(seed)) / 864 ** 0.5 * gain
  return w, torch.randn(1, generator=_gen(seed + 1)) * 0.1 * gain


def fwd_case(geom, gain=1.0):
  """x with sentinels (the activated volume of IN 0, the raw one of IN 1), w and bias times `gain` (1: a flat soft-max; 300: a
  saturated one), and the affine of the input BatchNorm"""
  B, D, H, W = geom
  x = add_sentinels(torch.randn(B, D, H, W, 32, generator=_gen(_seed(geom, 1))) * chan_scale())
  w, b = random_weights(_seed(geom, 2), gain)
  g = _gen(_seed(geom, 3))
  return dict(x=x, w=w, b=b, scale=1.0 + 0.5 * torch.randn(32, generator=g), shift=0.3 * torch.randn(32, generator=g))


def tap_weights(t, transposed=False):
  """forward: one channel of tap t is 1.0 (each logit is a shifted copy of that channel plus the bias); backward (transposed):
  every channel of tap t is +-2^k (g_a is a shifted copy of g_logits, scaled per channel by a power of two)"""
  w = torch.zeros(32, 27)
  if transposed:
    c = torch.arange(32)
    w[:, t] = torch.pow(2.0, (c % 5 - 2).float()) * (1.0 - 2.0 * (c % 2))
  else:
    w[(5 * t + 3) % 32, t] = 1.0
  return w.reshape(32, 3, 3, 3)


def tap_case(geom, t):
  """small integers in every channel, a single-tap weight and a bias that is a multiple of 2^-8: exact in fp32"""
  B, D, H, W = geom
  x = torch.randint(-8, 9, (B, D, H, W, 32), generator=_gen(_seed(geom, 4))).float()
  return dict(x=x, w=tap_weights(t), b=torch.tensor([(3 * t - 40) / 256.0]))


def designed_patterns(D):
  """name -> [D] logits: ties and extremes the index logic must get exactly right (those D has room for)"""
  def vec(pairs, fill=0.0):
    v = torch.full((D,), fill)
    for i, x in pairs:
      v[i] = x
    return v
  pats = {"all equal": vec([], 2.0)}
  if D >= 2:
    pats["maximum at D - 1"] = vec([(D - 1, 7.0)])
    pats["+-3e4"] = vec([(0, 3e4), (1, -3e4)])
  if D >= 3:
    pats["tie d, d + 1"] = vec([(1, 3.0), (2, 3.0)])
  if D >= 4:
    pats["three-way tie"] = vec([(0, 1.0), (1, 5.0), (2, 5.0), (D - 1, 5.0)])
    pats["duplicate maximum"] = vec([(0, 4.0), (1, 4.0), (2, 1.0)])
  if D >= 9:
    pats["tie 7, 8 (lanes 7 and 0)"] = vec([(7, 3.0), (8, 3.0)])
  if D >= 10:
    pats["tie d, d + 8 (one lane)"] = vec([(1, 7.0), (9, 7.0), (0, -2.0)])
  if D >= 26:
    pats["tie 1, 25 (k = 0 and 3)"] = vec([(1, 6.0), (25, 6.0)])
    pats["maximum at 24 and 31"] = vec([(24, 9.0), (31, 9.0), (30, 8.0)])
  return pats


def designed_case(geom, npos_wg):
  """integer logits driven through the centre tap of channel 0 (the convolution is then a copy: exact): a background of small
  integers (ties abound) and designed_patterns on the first pixels, on the last pixels of the last plane and inside the
  shifted-back last tile of the first image (tiles of npos_wg positions)"""
  B, D, H, W = geom
  l = torch.randint(-4, 5, (B, D, H, W), generator=_gen(_seed(geom, 5))).float()
  pats = designed_patterns(D)
  n = fwd_npos(H, W)
  yt, xt = divmod(n - max(npos_wg // 2, 1), W + 2)
  i_tile = yt * W + min(xt, W - 1)
  where = {}
  for k, (name, v) in enumerate(sorted(pats.items())):
    for tag, b, i in (("first", 0, k), ("last", B - 1, H * W - 1 - k), ("tile", 0, i_tile - k)):
      if 0 <= i < H * W:
        y, x = divmod(i, W)
        l[b, :, y, x] = v
        where[(name, tag)] = (b, y, x)
  x = torch.zeros(B, D, H, W, 32)
  x[..., 0] = l
  w = torch.zeros(32, 3, 3, 3)
  w[0, 1, 1, 1] = 1.0
  return dict(x=x, w=w, b=None, l=l, where=where)


def bwd_case(geom, gain=1.0):
  """logits with a standard deviation of 0.1 `gain` (flat to saturated), g_pred, g_in, the activation with sentinels, dense
  weights, and the prior values of an accumulating launch"""
  B, D, H, W = geom
  g = _gen(_seed(geom, 6))
  logits = torch.randn(B, D, H, W, generator=g) * 0.1 * gain
  g_pred, g_in = torch.randn(B, H, W, generator=g), torch.randn(B, D, H, W, generator=g) * 0.5
  a = add_sentinels(torch.randn(B, D, H, W, 32, generator=g) * chan_scale())
  w = random_weights(_seed(geom, 7))[0]
  return dict(logits=logits, g_pred=g_pred, g_in=g_in, a=a, w=w, gw0=torch.randn(32, 3, 3, 3, generator=g),
              gb0=torch.randn(1, generator=g))


BWD_SPOTS = ["corners", "seam"]


def bwd_exact_case(geom, t, spot, xc=13):
  """g_pred = None and g_in small integers: the logits gradient IS g_in.  w: tap t alone (+-2^k per channel): g_a is a shifted
  copy.  a: +-2^k per channel at TWO voxels — "corners": the first and the last voxel; "seam": either side of the first chunk
  seam (columns xc - 1 and xc, or the last two) on a middle row — so g_w sums two exact products; g_bias is an integer sum.
  Priors are multiples of 2^-8."""
  B, D, H, W = geom
  g = _gen(_seed(geom, 8))
  g_in = torch.randint(-4, 5, (B, D, H, W), generator=g).float()
  logits = torch.randn(B, D, H, W, generator=g)
  c = torch.arange(32)
  x1, x2 = min(xc - 1, max(W - 2, 0)), min(xc, W - 1)
  spots = {"corners": [(0, 0, 0, 0), (B - 1, D - 1, H - 1, W - 1)],
           "seam": [(0, D // 2, H // 2, x1), (B - 1, D // 2, H // 2, x2)]}[spot]
  a = torch.zeros(B, D, H, W, 32)
  a[spots[0]] = torch.pow(2.0, (c % 5 - 2).float()) * (1.0 - 2.0 * (c % 2))
  a[spots[1]] = a[spots[1]] + torch.pow(2.0, (c % 3 - 1).float()) * (1.0 - 2.0 * ((c // 2) % 2))
  gw0 = (torch.randn(32, 3, 3, 3, generator=g) * 256).round() / 256
  gb0 = (torch.randn(1, generator=g) * 256).round() / 256
  return dict(logits=logits, g_pred=None, g_in=g_in, a=a, w=tap_weights(t, True), gw0=gw0, gb0=gb0, spots=spots)


def cv_case(geom):
  """L, R [B, 32, H, W] and a volume gradient [B, D, H, W, 32], with per-channel scales"""
  B, D, H, W = geom
  g = _gen(_seed(geom, 9))
  cs = chan_scale()
  L, R = torch.randn(B, 32, H, W, generator=g) * cs.reshape(1, 32, 1, 1), torch.randn(B, 32, H, W, generator=g) * cs.reshape(1, 32, 1, 1)
  return dict(L=L, R=R, gvol=torch.randn(B, D, H, W, 32, generator=g) * cs)


# ----------------------------------------------------------------------------- deliberately wrong restatements
# name -> (stage, mut); tests/test_tail_ref_cpu.py shows that the cases above catch each of them
MUTANTS = {
  "a tap offset one row off (tap 5)": ("logits", ("row_off", 5)),
  "a tap offset one row off (tap 24)": ("logits", ("row_off", 24)),
  "the last tile not shifted back: its pixels unwritten": ("logits", ("no_shift_back", None)),
  "the pass over the zero plane skipped: the last logit never completed": ("logits", ("skip_zero_plane", 1)),
  "lane layout d = j + 8 k wrong beyond k = 2": ("soft", "lane_k3"),
  "the last maximum wins a tie": ("soft", "last_tie"),
  "FCS drops the duplicate of the maximum": ("soft", "fcs_no_dup"),
  "soft-max without subtracting the maximum": ("soft", "no_max"),
  "backward: the staged column x0 - 1 of a chunk taken as zero": ("bwd", ("col_zero", 1)),
  "backward: plane -1 of the gradient window not zero": ("bwd", ("plane_rep", "lo")),
  "backward: plane D of the gradient window not zero": ("bwd", ("plane_rep", "hi")),
  "backward: a unit skipped when a workgroup takes its second unit": ("bwd", ("skip_second_unit", 1)),
}
