"""A plain float64 restatement of ONE launch each of the feature head's 5x5 stride-2 layers (csrc/conv4_mfma.hip: the 3 -> 32
first layer; csrc/conv32_mfma.hip and csrc/conv32_s2.hip: the 32 -> 32 layers): forward, data gradient, weight and bias
gradient, the bound of each, and the cases the GPU file (tests/test_gpu_head_fp64.py) runs.  CPU only: nothing here imports
the library.  tests/test_head_ref_cpu.py holds the restatements to torch's float64 autograd, brackets two fp32 emulations with
the bounds and shows that the cases tell deliberately wrong restatements from the right one.

Tensors are channel-last: maps are [B, H, W, C] (a PCL interior with D = 1), weights are torch's [co][ci][5][5]; fp32 operands
are taken as they are and widened.  An input extent n gives the output extent (n - 1) // 2 + 1 (kernel 5, stride 2, padding 2).

Every bound is trunk_ref's rule, derived and never tuned: a sum of n terms added in ANY order in fp32 errs by at most
gamma(n) sum|terms|, sum|terms| being the same convolution on absolute values.
  forward         n = Cin * 25 + 1 (the products and the bias)
  data gradient   n = 32 * the taps of the output's parity phase: 9 / 6 / 6 / 4 for (y & 1, x & 1) = (0,0) (0,1) (1,0) (1,1)
  weight gradient n = B * Ho * Wo, every voxel of the launch (+ 1 with accumulate = 1: the value already there); the split
                  over waves, row segments and slabs does not enter, the rule holds for any order.

The functions that do the sums take a dtype and a `mut`: the float64 restatement is mut = None; the float32 run of the same
loop is the tap-by-tap emulation in the kernels' tap order; a `mut` is a deliberately WRONG restatement (MUTANTS), each a
mistake an index path of the kernels could make."""
import torch
import torch.nn.functional as F

import bn_ref as br
from trunk_ref import U, gamma_n    # noqa: F401

TAPS = [(j, l) for j in range(5) for l in range(5)]          # the forward kernels' order: tp = 5 ky + kx
PHASES = [(0, 0), (0, 1), (1, 0), (1, 1)]                    # (py, px) in as_conv32_dgrad_s2_pack's order
NAN = float("nan")


def out_extent(n):
  return (n - 1) // 2 + 1


def phase_taps(py, px):
  """the taps (j, l) of one parity phase, in the data gradient's order"""
  return [(j, l) for j in range(py, 5, 2) for l in range(px, 5, 2)]


def seg_steps(Wo, nseg):
  """pair-steps per row segment of the generic weight gradient, given the segments per row (as_conv32_wgrad_segments): the
  even split rounded up to the load groups of 8"""
  nsteps = (Wo + 1) // 2
  return ((nsteps + nseg - 1) // nseg + 7) // 8 * 8


# ----------------------------------------------------------------------------- the three sums
def fwd_sum(x, w, b, dtype=torch.float64, mut=None):
  """z[b, y, x, co] = bias[co] + sum_{ky, kx, ci} x[b, 2y + ky - 2, 2x + kx - 2, ci] w[co, ci, ky, kx], x zero outside the map;
  the accumulator starts at the bias and takes the taps in TAPS order.  x sits in a zero halo of 2 (the kernels' minimum).
  mut:  ("clamp_early", 1)    the staged kernels' right-edge clamp one voxel early: no padded column beyond W + 2 is read
        ("swap_halves", tap)  that tap reads the other column-parity half of the staged row: column offset kx ^ 1
        ("row_off", tap)      that tap's offset is one row down"""
  B, H, W, _ = x.shape
  Ho, Wo = out_extent(H), out_extent(W)
  xp = F.pad(x.to(dtype), (0, 0, 2, 4, 2, 4))               # padded coordinates: + 2; two more behind for the mutants
  z = b.to(dtype).reshape(1, 1, 1, -1).repeat(B, Ho, Wo, 1)
  ys, xs = 2 * torch.arange(Ho), 2 * torch.arange(Wo)
  kind, arg = mut if mut is not None else (None, None)
  for (ky, kx) in TAPS:
    if not bool(w[:, :, ky, kx].any()):                      # (a single-tap case: the other taps add exact zeros)
      continue
    dy, dx = ky, kx
    if kind == "swap_halves" and arg == (ky, kx):
      dx = kx ^ 1
    if kind == "row_off" and arg == (ky, kx):
      dy = ky + 1
    cols = xs + dx
    if kind == "clamp_early":
      cols = cols.clamp(max=W + 3 - arg)
    a = xp[:, ys + dy][:, :, cols]
    z = z + torch.einsum("bhwi,oi->bhwo", a, w[:, :, ky, kx].to(dtype))
  return z


def dgrad_sum(gz, w, H, W, dtype=torch.float64, pz=1, mut=None):
  """The adjoint of fwd_sum in x, the way the kernels form it: the output pixel (2y' + py, 2x' + px) of phase (py, px) sums
  its taps (j, l) in phase_taps order over gz[y' + (py + 2 - j) / 2, x' + (px + 2 - l) / 2], gz zero outside its map, and is
  stored where 2y' + py < H and 2x' + px < W.  Returns g_x inside a halo of 1 that holds NaN: what was never stored, and what
  a launch must leave alone.  pz: gz's own halo (it decides what a clamped column holds).
  mut:  ("clamp_early", 1)  the staged kernel's right-edge clamp one voxel early: no padded gz column beyond Wz + 2 pz - 2
        ("store_le_H", 1)   a phase stored where 2y' + py <= H
        ("row_off", tap)    that tap reads one coarse row further down"""
  B, Hz, Wz, _ = gz.shape
  assert Hz == out_extent(H) and Wz == out_extent(W)
  kind, arg = mut if mut is not None else (None, None)
  gp = F.pad(gz.to(dtype), (0, 0, pz, pz + 2, pz, pz + 2))   # padded coordinates: + pz
  out = torch.full((B, H + 2, W + 2, w.shape[1]), NAN, dtype=dtype)
  yc, xc = torch.arange(Hz), torch.arange(Wz)
  for (py, px) in PHASES:
    acc = torch.zeros(B, Hz, Wz, w.shape[1], dtype=dtype)
    for (j, l) in phase_taps(py, px):
      if not bool(w[:, :, j, l].any()):
        continue
      oy, ox = (py + 2 - j) // 2, (px + 2 - l) // 2
      if kind == "row_off" and arg == (j, l):
        oy += 1
      cols = xc + ox + pz
      if kind == "clamp_early":
        cols = cols.clamp(max=Wz + 2 * pz - 1 - arg)
      a = gp[:, yc + oy + pz][:, :, cols]
      acc = acc + torch.einsum("bhwo,oi->bhwi", a, w[:, :, j, l].to(dtype))
    hlim = H + 1 if kind == "store_le_H" else H
    ny, nx = min(len(range(py, hlim, 2)), Hz), len(range(px, W, 2))
    out[:, 1 + py:1 + py + 2 * ny:2, 1 + px:1 + px + 2 * nx:2] = acc[:, :ny, :nx]
  return out


def wgrad_sum(x, gz, dtype=torch.float64, mut=None, nseg=1):
  """dW[co, ci, ky, kx] = sum_{b, y, x} x[b, 2y + ky - 2, 2x + kx - 2, ci] gz[b, y, x, co]  and  db[co] = sum gz.
  mut:  ("unmasked_second", 1)  the second voxel of a row's last pair-step is not masked where Wo is odd: its clamped address
                                is the last column, which then counts twice
        ("seam_twice", 1)       the first pair-step of the second segment is also the last of the first (nseg from the launch)"""
  B, H, W, _ = x.shape
  _, Ho, Wo, _ = gz.shape
  kind, arg = mut if mut is not None else (None, None)
  mult = torch.ones(Wo, dtype=dtype)
  if kind == "unmasked_second" and Wo % 2 == 1:
    mult[Wo - 1] += 1
  if kind == "seam_twice" and nseg > 1:
    s = seg_steps(Wo, nseg)
    mult[2 * s:2 * s + 2] += 1
  g = gz.to(dtype) * mult.reshape(1, 1, Wo, 1)
  xp = F.pad(x.to(dtype), (0, 0, 2, 3, 2, 3))
  dW = torch.zeros(gz.shape[3], x.shape[3], 5, 5, dtype=dtype)
  for (ky, kx) in TAPS:
    dW[:, :, ky, kx] = torch.einsum("bhwo,bhwi->oi", g, xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2])
  return dW, g.sum((0, 1, 2))


# ----------------------------------------------------------------------------- restatement + bound
def forward(x, w, b):
  """z and its bound:  e = gamma(Cin * 25 + 1) (conv(|x|, |w|) + |b|)"""
  n = x.shape[3] * 25 + 1
  return dict(z=fwd_sum(x, w, b), e_z=gamma_n(n) * fwd_sum(x.abs(), w.abs(), b.abs()))


def phase_terms(H, W):
  """[H, W]: the number of terms of a data-gradient output, 32 * taps of its parity phase"""
  ty = 3 - (torch.arange(H) % 2)
  tx = 3 - (torch.arange(W) % 2)
  return 32 * ty[:, None] * tx[None, :]


def data_gradient(gz, w, H, W, pz=1):
  """g_x (inside the NaN halo of dgrad_sum) and its bound (interior only):  e = gamma(32 taps(py, px)) dgrad(|gz|, |w|)"""
  g = dgrad_sum(gz, w, H, W, pz=pz)
  s = dgrad_sum(gz.abs(), w.abs(), H, W, pz=pz)[:, 1:-1, 1:-1]
  n = phase_terms(H, W).double()
  gam = (n * U / (1.0 - n * U)).reshape(1, H, W, 1)
  return dict(g_x=g, e_g_x=gam * s)


def weight_gradient(x, gz, dW0=None, db0=None):
  """dW, db and their bounds  e = gamma(N) wgrad(|x|, |gz|),  gamma(N) sum|gz|,  N = B Ho Wo.  With dW0 / db0 (accumulate = 1)
  the value already there is one more term: N + 1, and its magnitude joins the sum."""
  N = gz.shape[0] * gz.shape[1] * gz.shape[2]
  dW, db = wgrad_sum(x, gz)
  aW, ab = wgrad_sum(x.abs(), gz.abs())
  if dW0 is not None:
    N += 1
    dW, db = dW + dW0.double(), db + db0.double()
    aW, ab = aW + dW0.double().abs(), ab + db0.double().abs()
  return dict(dW=dW, db=db, e_dW=gamma_n(N) * aW, e_db=gamma_n(N) * ab)


# ----------------------------------------------------------------------------- judging
def ratio(got, ref, bound):
  """worst |got - ref| / bound; a NaN in got (an element never written, or a guard value consumed) counts as infinite"""
  got, ref = got.double().reshape(ref.shape), ref.double()
  if bool(torch.isnan(got).any()):
    return float("inf")
  return br.worst_ratio((got - ref).abs(), bound.double().reshape(ref.shape))


def halo_kept(padded):
  """dgrad_sum's output: every halo element still NaN"""
  p = padded.clone()
  p[:, 1:-1, 1:-1] = NAN
  return bool(torch.isnan(p).all())


# ----------------------------------------------------------------------------- the geometries the GPU file runs
# The first layer: (B, H, W) of the image and whether as_conv4_s2_ok (tiles = B Ho ceil(Wo / 32) >= 4096)
CONV4_GEOMS = [
  ((64, 127, 63), 1),     # 4096 tiles exactly: two full rounds of the 2048 persistent waves; odd / odd; the clamp on a full segment
  ((64, 128, 64), 1),     # even / even
  ((43, 96, 65), 1),      # 4128: a second segment of one column whose last tap reads the last padded voxel; ragged third round
  ((63, 127, 63), 0),     # 4032, just below: the one-tile kernel
  ((1, 9, 13), 0),
  ((2, 5, 131), 0),       # Wo = 66: weight-gradient units of 64 pixels, two per row
]
# 32 -> 32 forward: (B, H, W) of the input and the route (M = B Ho Wo; split-K takes M <= 16384; staged rows from 1024 tiles)
FWD_GEOMS = [
  ((32, 63, 33), "staged"),     # 1024 tiles, M = 17408: the threshold exactly, odd / odd
  ((32, 63, 31), "splitk"),     # 1024 tiles, M = 16384: split-K has precedence
  ((16, 64, 66), "staged"),     # even / even, a last segment of one column
  ((17, 61, 130), "staged"),    # 1581 tiles: the last workgroup has one live wave
  ((31, 63, 33), "direct"),     # 992 tiles, M = 16864
  ((3, 21, 33), "splitk"),      # M = 561: a ragged last 32-voxel tile
]
# data gradient: (B, H, W) of g_x and whether the staged kernel takes it (tiles of g_z >= 1024)
DGRAD_GEOMS = [
  ((32, 63, 33), 1), ((32, 64, 34), 1), ((16, 64, 65), 1), ((16, 63, 66), 1),
  ((31, 63, 33), 0), ((31, 64, 34), 0), ((31, 64, 33), 0), ((31, 63, 34), 0),      # 992 tiles: the generic four-phase kernel
  ((1, 1, 1), 0), ((1, 2, 2), 0), ((1, 5, 7), 0),                                  # degenerate phases
]
# weight gradient of the 32 -> 32 layers: (B, H, W) of x and the segments per row
WGRAD_GEOMS = [
  ((1, 9, 13), 1),
  ((1, 5, 131), 2),       # Wo = 66: 24 + 9 pair-steps, a ragged last segment
  ((2, 7, 133), 2),       # Wo = 67: an odd last column in segment 1
  ((2, 94, 311), 3),      # 47 x 156: 32 / 32 / 14, the level one pair per step runs
  ((5, 79, 131), 2),      # 1000 row-waves
  ((5, 81, 131), 1),      # 1025
]


def geom_id(g):
  return "%dx%dx%d" % tuple(g)


# ----------------------------------------------------------------------------- the cases
def _gen(seed):
  return torch.Generator().manual_seed(seed)


def _seed(geom, k):
  B, H, W = geom
  return 100003 * k + 7 * B + 131 * H + W


def chan_scale(C):
  """different magnitudes per channel, so that a channel swizzle fails"""
  return torch.pow(2.0, (torch.arange(C) % 5 - 2).float())


def add_sentinels(t):
  """+-1e4 in one channel each at the corners and the edge midpoints of the first and the last image: a value that reaches an
  output it does not belong to moves it orders beyond the bound"""
  B, H, W, C = t.shape
  spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]
  for bi in sorted({0, B - 1}):
    for k, (y, x) in enumerate(spots):
      t[bi, y, x, (5 * k + 3 * bi) % C] = 1e4 * (-1.0) ** (k + bi)
  return t


def random_weights(cin, seed):
  w = torch.randn(32, cin, 5, 5, generator=_gen(seed)) / (cin * 25) ** 0.5
  return w, torch.randn(32, generator=_gen(seed + 1)) * 0.1


def tap_weights(cin, t, transposed=False):
  """One tap times a channel permutation: w[co, perm[co], tap] = +-2^k, zero elsewhere (cin < 32: w[co, co % cin]).  The
  forward (transposed: the data gradient, which sums over co) is then a copy of x scaled by a power of two: exact."""
  ky, kx = TAPS[t]
  w = torch.zeros(32, cin, 5, 5)
  co = torch.arange(32)
  perm = torch.randperm(32, generator=_gen(50 + t)) if cin == 32 else co % cin
  val = torch.pow(2.0, (co % 7 - 3).float()) * (1.0 - 2.0 * (co % 2))
  w[co, perm, ky, kx] = val
  return w


def fwd_case(geom, fam, cin=32):
  """x with sentinels, and: fam "random": dense weights and bias; ("tap", t): tap_weights, no bias"""
  B, H, W = geom
  x = torch.randn(B, H, W, cin, generator=_gen(_seed(geom, 1))) * chan_scale(cin)
  add_sentinels(x)
  if fam == "random":
    w, b = random_weights(cin, _seed(geom, 2))
  else:
    w, b = tap_weights(cin, fam[1]), torch.zeros(32)
  return dict(x=x, w=w, b=b)


def dgrad_case(geom, fam):
  """g_z with sentinels for a g_x of extent geom; weights as fwd_case"""
  B, H, W = geom
  gz = torch.randn(B, out_extent(H), out_extent(W), 32, generator=_gen(_seed(geom, 3))) * chan_scale(32)
  add_sentinels(gz)
  w = random_weights(32, _seed(geom, 4))[0] if fam == "random" else tap_weights(32, fam[1])
  return dict(gz=gz, w=w)


IMPULSE_SPOTS = ["seam", "last_col", "rows"]


def wgrad_case(geom, fam, cin=32, nseg=1, seam=None):
  """fam "random": x and g_z dense with sentinels.  ("impulse", spot): g_z is +-2^k per channel at TWO voxels and x holds
  multiples of 2^-8 below 16, so every dW entry is a sum of two products that fp32 holds exactly in any order.  Spots:
  "seam" the last pair-step of segment 0 and the first of segment 1 (`seam`: the pair-steps of a segment where the kernel does
  not cut by seg_steps; mid-row where there is one segment); "last_col" the last
  column of the first and the last row; "rows" the first row of the first image and the last row of the last."""
  B, H, W = geom
  Ho, Wo = out_extent(H), out_extent(W)
  gen = _gen(_seed(geom, 5))
  if fam == "random":
    x = add_sentinels(torch.randn(B, H, W, cin, generator=gen) * chan_scale(cin))
    gz = add_sentinels(torch.randn(B, Ho, Wo, 32, generator=gen) * chan_scale(32))
    return dict(x=x, gz=gz)
  x = (torch.randn(B, H, W, cin, generator=gen) * 256.0).round().clamp(-4095, 4095) / 256.0
  s = seam if seam is not None else (seg_steps(Wo, nseg) if nseg > 1 else max((Wo + 1) // 4, 1))
  c0, c1 = min(2 * s - 1, Wo - 1), min(2 * s, Wo - 1)
  spots = {"seam": [(0, Ho // 2, c0), (0, Ho // 2, c1)],
           "last_col": [(0, 0, Wo - 1), (B - 1, Ho - 1, Wo - 1)],
           "rows": [(0, 0, Wo // 3), (B - 1, Ho - 1, (2 * Wo) // 3)]}[fam[1]]
  co = torch.arange(32)
  gz = torch.zeros(B, Ho, Wo, 32)
  gz[spots[0]] = torch.pow(2.0, (co % 5 - 2).float()) * (1.0 - 2.0 * (co % 2))
  gz[spots[1]] = gz[spots[1]] + torch.pow(2.0, (co % 3 - 1).float()) * (1.0 - 2.0 * ((co // 2) % 2))
  return dict(x=x, gz=gz, spots=spots)


# ----------------------------------------------------------------------------- deliberately wrong restatements
# name -> (op, mut); tests/test_head_ref_cpu.py shows that the cases above catch each of them
MUTANTS = {
  "right-edge clamp one voxel early (data gradient, g_z halo 1)": ("dgrad", ("clamp_early", 1)),
  "column-parity halves swapped for tap (2, 3)": ("fwd", ("swap_halves", (2, 3))),
  "column-parity halves swapped for tap (0, 4)": ("fwd", ("swap_halves", (0, 4))),
  "data-gradient phase stored at yo <= H": ("dgrad", ("store_le_H", 1)),
  "last pair-step's second voxel not masked": ("wgrad", ("unmasked_second", 1)),
  "segment seam counted twice": ("wgrad", ("seam_twice", 1)),
  "forward tap (4, 0) off by a row": ("fwd", ("row_off", (4, 0))),
  "data-gradient tap (0, 2) off by a row": ("dgrad", ("row_off", (0, 2))),
}
