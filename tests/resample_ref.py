"""fp64 reference of bilinear resampling with align_corners=False (csrc/resample.hip: as_upsample_bilinear_fwd / _bwd), and the
bound a float32 evaluation of it has to keep.

The operation is separable, so one case is two small dense matrices: out = gain * Wy S Wx^T, adjoint = gain * Wy^T G Wx.

Coordinates.  ``coords(n, N)`` is ATen's sequence in float32, op by op and unfused: ``scale = float(n) / float(N)``,
``r = max(scale * (d + 0.5) - 0.5, 0)``, ``i0 = min(int(r), n - 1)``, ``i1 = i0 + (i0 < n - 1)``, ``l1 = r - i0``.  The matrices take
these float32 coordinates as given (the cell of every destination index is the float32 cell) and are float64 from there on:
``W[d, i0] += 1 - l1``, ``W[d, i1] += l1`` (added, so a clamped tap carries weight 1).

What a different rounding of the coordinate can do is bounded instead of reproduced.  The only rounded step of ``r`` is the
product ``t = scale * (d + 0.5)`` (``t - 0.5`` is exact in binary32: the result is a multiple of t's ulp and not larger than
t), so a fused multiply-add and the unfused sequence both lie within half an ulp of t of the exact value, and differ from each
other by at most ``ulp32(t) = ulp32(r + 0.5)``.  A weight's derivative in ``r`` is -1 at i0 and +1 at i1 (0 where the two
coincide), so ``|D|[d, i]`` is 1 at each distinct tap, and ``E = |D| * ulp32(r + 0.5)`` in place of ``W`` on one axis bounds the
first-order effect of one ulp there.  Where the float32 ``r`` lies within 2 ulp of an integer k, the other evaluation may fall
into the neighbouring cell; the interpolant is continuous across k, so the difference is still (coordinate difference) x
(larger of the two cells' slopes), and ``|D|`` marks k - 1, k and k + 1 there.  Where the product is exact in binary32
(integer ratios: the halving pyramid, the identity) no evaluation rounds it and the term is zero.

Bounds, per element, ``U = 2^-24``:  ``K * U * mag + 2 * coord``.  ``mag`` is the same product with ``|S|`` / ``|G|``; ``coord``
the same product with ``E`` in place of ``W`` on one axis at a time, both axes added.  The factor 2: each of the two
evaluations is one ulp from the other at most, and torch's own CPU kernel already reaches 0.99 of one ulp at 375 x 1242.
K counts the roundings one term passes through:

* forward ``K_FWD = 5``: the two blends along x, the blend along y, the gain, and one for ``l0 = 1 - l1`` (formed in float32
  by the kernel, exact here);
* backward ``ny + ceil(nx / 64) + 6 + 4``: pass 1 adds the ``ny`` footprint rows of a coarse row one after the other, pass 2
  adds ``ceil(nx / 64)`` terms per lane and then a 6-level tree over the wave, and 4 for the two weights, their products and
  the gain; ``ny`` / ``nx`` are the largest numbers of non-zero entries in a column of ``Wy`` / ``Wx``.

``widen=True`` adds the float-vs-double difference of ``scale`` itself, ``(r + 0.5) * 2^-24``, to the one ulp: that is the
distance to an evaluation whose coordinates are float64 throughout (F.interpolate on a float64 tensor), used by the CPU test
to check the neighbouring-cell refinement.
"""
import math

import torch

U = 2.0 ** -24
K_FWD = 5
F32, F64 = torch.float32, torch.float64


def ulp32(x):
  """spacing of binary32 at |x| (x a float32 tensor of normal numbers) -> float64"""
  return torch.pow(2.0, torch.frexp(x.float()).exponent.double() - 24.0)


def coords(n, N):
  """ATen's float32 source coordinates of the N destination indices over a source of n -> dict(scale, t, r, i0, i1, l1);
  t = scale * (d + 0.5) is the one rounded product, r = max(t - 0.5, 0)"""
  scale = torch.tensor(float(n), dtype=F32) / torch.tensor(float(N), dtype=F32)
  d = torch.arange(N, dtype=F32)
  t = scale * (d + 0.5)
  r = (t - 0.5).clamp_min(0.0)
  i0 = r.to(torch.int64).clamp_max(n - 1)
  i1 = i0 + (i0 < n - 1).to(torch.int64)
  l1 = r - i0.to(F32)
  return dict(scale=scale, t=t, r=r, i0=i0, i1=i1, l1=l1)


def matrices(n, N, widen=False):
  """(W, E): the float64 interpolation matrix [N, n] from the float32 coordinates, and |D| * coordinate-ulp (see the module's
  docstring)"""
  c = coords(n, N)
  ar = torch.arange(N)
  i0, i1, l1 = c["i0"], c["i1"], c["l1"].double()
  W = torch.zeros(N, n, dtype=F64)
  W.index_put_((ar, i0), 1.0 - l1, accumulate=True)
  W.index_put_((ar, i1), l1, accumulate=True)
  D = torch.zeros(N, n, dtype=F64)
  two = (i1 != i0).double()
  D[ar, i0] = two
  D[ar, i1] = two
  delta = ulp32(c["t"])
  exact = c["scale"].double() * (torch.arange(N, dtype=F64) + 0.5) == c["t"].double()      # (24 x 24 bits: exact in float64)
  delta = torch.where(exact, torch.zeros_like(delta), delta)
  raw = c["t"].double() - 0.5
  k = torch.round(raw)
  near = ((raw - k).abs() <= 2.0 * delta) & (k >= 0)
  kk = k.to(torch.int64).clamp(0, n - 1)
  for off in (-1, 0, 1):
    col = (kk + off).clamp(0, n - 1)
    D[ar[near], col[near]] = 1.0
  if widen:
    delta = delta + c["t"].double() * U
  return W, D * delta[:, None]


def _gain32(gain):
  return float(torch.tensor(float(gain), dtype=F32))


def forward(src, H, W, gain, widen=False):
  """src [B, h, w] -> (reference [B, H, W], bound [B, H, W], coord [B, H, W]) in float64; bound = K_FWD U mag + 2 coord"""
  g = _gain32(gain)
  S = src.detach().cpu().double()
  Wy, Ey = matrices(S.shape[1], H, widen)
  Wx, Ex = matrices(S.shape[2], W, widen)
  A = S.abs()
  ref = g * (Wy @ S @ Wx.t())
  mag = abs(g) * (Wy @ A @ Wx.t())
  coord = abs(g) * (Ey @ A @ Wx.t() + Wy @ A @ Ex.t())
  return ref, K_FWD * U * mag + 2.0 * coord, coord


def k_bwd(h, w, H, W):
  """(K, ny, nx) of the backward's bound for a coarse (h, w) and a fine (H, W)"""
  ny = int((matrices(h, H)[0] != 0).sum(0).max())
  nx = int((matrices(w, W)[0] != 0).sum(0).max())
  return ny + int(math.ceil(nx / 64.0)) + 6 + 4, ny, nx


def adjoint(g_dst, h, w, gain, widen=False):
  """g_dst [B, H, W] -> (reference [B, h, w], bound, coord) in float64; bound = K U mag + 2 coord with K = k_bwd(...)"""
  g = _gain32(gain)
  G = g_dst.detach().cpu().double()
  H, W = G.shape[1], G.shape[2]
  Wy, Ey = matrices(h, H, widen)
  Wx, Ex = matrices(w, W, widen)
  A = G.abs()
  ref = g * (Wy.t() @ G @ Wx)
  mag = abs(g) * (Wy.t() @ A @ Wx)
  coord = abs(g) * (Ey.t() @ A @ Wx + Wy.t() @ A @ Ex)
  K = k_bwd(h, w, H, W)[0]
  return ref, K * U * mag + 2.0 * coord, coord


def worst_ratio(got, ref, bound):
  """max |got - ref| / bound over the elements (0 / 0 counts as 0, x / 0 as inf)"""
  err = (got.detach().cpu().double() - ref).abs()
  ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
  return float(ratio.max()) if ratio.numel() else 0.0


# ----------------------------------------------------------------------------------------------------------------------------
# float32 emulations of the kernel's own arithmetic (CPU test only: they keep the bound honest without a GPU)
# ----------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
  """a * b + c rounded once to float32 (the exact product and one addition in float64, then to float32)"""
  return (a.double() * b.double() + c.double()).float()


def coords_kernel(n, N, fused):
  """bilin_src() of csrc/resample.hip in float32: as coords(), the coordinate a fused multiply-add when ``fused``"""
  scale = torch.tensor(float(n), dtype=F32) / torch.tensor(float(N), dtype=F32)
  d = torch.arange(N, dtype=F32) + 0.5
  r = _fma(scale.expand_as(d), d, torch.full_like(d, -0.5)) if fused else scale * d - 0.5
  r = r.clamp_min(0.0)
  i0 = r.to(torch.int64).clamp_max(n - 1)
  i1 = i0 + (i0 < n - 1).to(torch.int64)
  l1 = r - i0.to(F32)
  return i0, i1, 1.0 - l1, l1


def forward_kernel_order(src, H, W, gain, fused):
  """upsample_fwd_kernel's expression in float32: top / bot = lx0 * a + lx1 * b, out = (ly0 * top + ly1 * bot) * gain, with
  every multiply-add contracted (``fused``) or every operation rounded"""
  S = src.float()
  g = torch.tensor(float(gain), dtype=F32)
  y0, y1, ly0, ly1 = coords_kernel(S.shape[1], H, fused)
  x0, x1, lx0, lx1 = coords_kernel(S.shape[2], W, fused)

  def blend(a0, a, a1, b):
    return _fma(a0, a, a1 * b) if fused else a0 * a + a1 * b
  top = blend(lx0, S[:, y0][:, :, x0], lx1, S[:, y0][:, :, x1])
  bot = blend(lx0, S[:, y1][:, :, x0], lx1, S[:, y1][:, :, x1])
  return blend(ly0[None, :, None], top, ly1[None, :, None], bot) * g


def footprint32(n, N, tighten=0):
  """footprint() of csrc/resample.hip in float32 for every coarse index i -> (lo [n], hi [n]) int64, clipped to [0, N - 1];
  ``tighten`` moves both ends inwards by that many indices"""
  scale = torch.tensor(float(n), dtype=F32) / torch.tensor(float(N), dtype=F32)
  i = torch.arange(n, dtype=F32)
  lo = torch.floor((i - 1.0 + 0.5) / scale - 0.5).to(torch.int64) - 1 + tighten
  hi = torch.ceil((i + 1.0 + 0.5) / scale - 0.5).to(torch.int64) + 1 - tighten
  return lo.clamp_min(0), hi.clamp_max(N - 1)


# ----------------------------------------------------------------------------------------------------------------------------
# the shapes of tests/test_gpu_resample_fp64.py, (h, w, H, W, gain): source (h, w), destination (H, W); the CPU test holds the
# reference to torch at every one of them
# ----------------------------------------------------------------------------------------------------------------------------
PRODUCTION = [(24, 78, 375, 1242), (34, 60, 540, 960), (10, 17, 75, 131), (47, 156, 375, 1242)]
PRODUCTION = [(h, w, H, W, W / w) for h, w, H, W in PRODUCTION]
PYRAMID_NO_LDS = [(375, 1242, 187, 621, 0.5), (375, 1242, 93, 310, 0.25), (375, 1242, 46, 155, 0.125)]
PYRAMID_LDS = [(320, 960, 160, 480, 0.5), (320, 960, 80, 240, 0.25), (320, 960, 40, 120, 0.125)]
TEMPLATE_SWITCH = [(5, 1024, 7, 1500, 1500 / 1024), (5, 1025, 7, 1500, 1500 / 1025)]
NARROW = [(3, 2, 5, W, W / 2) for W in range(1, 10)]
RESIDUES = [(5, 7, 9, W, W / 7) for W in (33, 34, 35, 36)]
WIDE = [(2, 50, 3, 4100, 82.0)]
ONE = [(1, 1, 5, 7, 7.0)]
TALL = [(2, 3, 600, 40, 40 / 3)]                      # backward: 600 / 2 * 2 footprint rows > 256, no row-weight table
CHUNK_ONE = [(3, 2, 5, 400, 200.0), (2, 3, 4, 1000, 1000 / 3)]          # backward: W / w in 85 .. 339
DOWN_ADJOINT = [(375, 1242, 47, 156, 0.125)]          # backward: the adjoint of a down-sampling
FWD_SHAPES = PRODUCTION + PYRAMID_NO_LDS + PYRAMID_LDS + TEMPLATE_SWITCH + NARROW + RESIDUES + WIDE + ONE
BWD_SHAPES = PRODUCTION + TALL + CHUNK_ONE + DOWN_ADJOINT + ONE + [(3, 2, 5, 9, 4.5), (5, 7, 9, 35, 5.0)]
ALL_SHAPES = sorted(set(FWD_SHAPES + BWD_SHAPES))
