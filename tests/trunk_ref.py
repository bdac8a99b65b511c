"""A plain float64 restatement of ONE launch of the feature trunk (csrc/trunk.hip) in each direction, and the error models the
GPU tests (tests/test_gpu_trunk_fp64.py) bound the kernels with.  CPU only: nothing here imports the library.  The BatchNorm
parts are bn_ref.py's.

Tensors are channel-last: maps are [B, H, W, 32] (a PCL interior with D = 1), weights are torch's [co][ci][3][3].  The leading
dimension splits into `groups` equal statistics groups (the left / right images of a pair).  A BatchNorm state is a dict of
mean / invstd / scale / shift, each [groups, 32]: the fp32 values the kernel published (or read), taken as they are.

Every bound is derived, none is tuned.  One rule carries most of them: a sum of n terms added in ANY order in fp32 (products
rounded or fused) errs by at most  gamma(n) sum|terms|,  gamma(n) = n U / (1 - n U), U = 2^-24 (Higham, Accuracy and Stability
of Numerical Algorithms, 2nd ed., section 3.1; n rather than n - 1 so that the rounding of each product is covered as well) —
the order in which the matrix instruction, the split over waves and the slab reduction add does not enter.  What a launch
forms but does not store (the staged operand of a BasicBlock forward, g_z of its backward) enters the sums that consume it with
its own bound, propagated through |w| (forward, data gradient) or |x| (weight gradient).  Each model is written next to the
function that returns it."""
import math

import torch
import torch.nn.functional as F

import bn_ref as br

U = br.U
SLOPE = br.SLOPE
K_BWD = 16               # the BatchNorm backward's sums and stage 3: the constant of tests/test_gpu_batchnorm_fp64.py part C
K_OP = 4                 # roundings of the staged operand lrelu(src*scale + shift) + skip: product, add, slope, add
TILE = 32                # a tile is 32 consecutive x of one row
GPER_MAX = 128           # workgroups per statistics group


def gamma_n(n):
  return n * U / (1.0 - n * U)


# ----------------------------------------------------------------------------- the launch geometry
def tiling(B, H, W, groups):
  """The kernels' split of a [B, H, W] map: tiles per row / per group, rounds, workgroups per group (`gper`, also the number
  of partials a launch leaves per group) and n_lane = 16 * rounds: one lane holds 16 voxels of each tile its workgroup runs.
  The last tile of a row is shifted left to end at W; `dup` is the overlap it re-computes (left out of every reduction)."""
  assert B % groups == 0
  tpr = (W + TILE - 1) // TILE
  tiles = (B // groups) * H * tpr
  rounds = (tiles + GPER_MAX - 1) // GPER_MAX
  gper = (tiles + rounds - 1) // rounds
  rounds_real = (tiles + gper - 1) // gper
  x0_last = min(TILE * (tpr - 1), max(W - TILE, 0))
  return dict(tiles_per_row=tpr, tiles_per_group=tiles, rounds=rounds_real, gper=gper, n_lane=16 * rounds_real,
              dup=TILE * (tpr - 1) - x0_last, seam=x0_last)


# ----------------------------------------------------------------------------- convolutions in float64
def _nchw(t):
  return t.double().permute(0, 3, 1, 2)


def conv64(a, w):
  """z[b, y, x, co] = sum_{ci, kh, kw} a[b, y + kh - 1, x + kw - 1, ci] w[co, ci, kh, kw], a zero outside the map"""
  return F.conv2d(_nchw(a), w.double(), padding=1).permute(0, 2, 3, 1)


def dgrad64(g_z, w):
  """the adjoint of conv64 in a:  g[b, y, x, ci] = sum_{co, kh, kw} g_z[b, y - kh + 1, x - kw + 1, co] w[co, ci, kh, kw]"""
  return F.conv_transpose2d(_nchw(g_z), w.double(), padding=1).permute(0, 2, 3, 1)


def wgrad64(x, g_z):
  """the adjoint of conv64 in w:  dW[co, ci, kh, kw] = sum_{b, y, x} x[b, y + kh - 1, x + kw - 1, ci] g_z[b, y, x, co]"""
  x, g_z = x.double(), g_z.double()
  B, H, W, _ = x.shape
  xp = F.pad(x, (0, 0, 1, 1, 1, 1))
  dW = torch.zeros(32, 32, 3, 3, dtype=torch.float64)
  for kh in range(3):
    for kw in range(3):
      dW[:, :, kh, kw] = torch.einsum("bhwo,bhwi->oi", g_z, xp[:, kh:kh + H, kw:kw + W])
  return dW


def split_state(state, gi):
  return {k: state[k][gi] for k in ("mean", "invstd", "scale", "shift")}


def state_from_kernel(st):
  """[groups, 5, 32] as trunk_bn_merge publishes it (mean, invstd, scale, shift, unbiased variance) -> state dict (+ var_u)"""
  st = st.detach().cpu()
  return dict(mean=st[:, 0], invstd=st[:, 1], scale=st[:, 2], shift=st[:, 3], var_u=st[:, 4])


CRAFT_BETA = 0.25        # beta of the crafted states: y = beta, not a rounding residue, where z sits on its mean (a 1 x 1 map)


def craft_state(z, gamma, groups, beta=None):
  """A state per group from z's fp64 moments, rounded to fp32 the way a finalize does (tests/test_gpu_batchnorm_fp64.py's
  _state64): mean, invstd, scale = invstd * gamma and shift = beta - mean * scale in fp32.  Returns the dict and the
  [groups, 5, 32] fp32 tensor the kernels read (slot 4, the unbiased variance, included)."""
  zg = z.reshape(groups, -1, 32).double()
  mean = zg.mean(1).float()
  var = zg.var(1, unbiased=False)
  invstd = (1.0 / torch.sqrt(var + br.EPS)).float()
  scale = invstd * gamma.float()
  shift = (beta.float() if beta is not None else torch.zeros(32)) - mean * scale
  n = zg.shape[1]
  var_u = (var * (n / (n - 1.0) if n > 1 else 1.0)).float()
  return dict(mean=mean, invstd=invstd, scale=scale, shift=shift), torch.stack([mean, invstd, scale, shift, var_u], 1).contiguous()


# ----------------------------------------------------------------------------- forward layer
def forward_layer(src, w, bias, skip=None, state=None, groups=1, slope=SLOPE):
  """One forward launch.  MODE 0 (state None): the operand a is src.  MODE 1: a = lrelu(src * scale + shift) + skip with the
  group's scale / shift, the branch from bn_ref.lrelu_branch (the fma form; `amb` lists the elements whose branch depends on
  it).  z = conv64(a) + bias with zero padding OF a (a BatchNorm'd zero would be lrelu(shift)).

  Model.  a: the kernel rounds the product (or fuses it), the add, the slope and the add of skip: at most K_OP = 4 roundings of
  values no larger than |src*scale| + |shift| + |skip|:
      e_a = K_OP U (|src*scale| + |shift| + |skip|)        (+ on an ambiguous branch, where |y| is itself a rounding error of
                                                             src*scale + shift: (1 - slope)(|y| + 2 U (|src*scale| + |shift|)))
  z: 288 products and the bias, n = 289 terms:
      e_z = gamma(289) (conv(|a|, |w|) + |bias|) + conv(e_a, |w|)"""
  src = src.double()
  w64, aw = w.double(), w.double().abs()
  n_amb = 0
  amb = torch.zeros(src.shape, dtype=torch.bool)
  if state is None:
    a, e_a = src, torch.zeros_like(src)
  else:
    B = src.shape[0]
    per = B // groups
    a, e_a = torch.empty_like(src), torch.empty_like(src)
    for gi in range(groups):
      sl = slice(gi * per, (gi + 1) * per)
      sc, sh = state["scale"][gi].double(), state["shift"][gi].double()
      pos, am = br.lrelu_branch(src[sl], sc, sh)
      y = src[sl] * sc + sh
      mag = (src[sl] * sc).abs() + sh.abs()
      a[sl] = torch.where(pos, y, y * slope) + skip[sl].double()
      e_a[sl] = K_OP * U * (mag + skip[sl].double().abs()) + \
          torch.where(am, (1.0 - slope) * (y.abs() + 2.0 * U * mag), torch.zeros_like(y))
      amb[sl] = am
    n_amb = int(amb.sum())
  z = conv64(a, w64) + bias.double()
  e_z = gamma_n(289) * (conv64(a.abs(), aw) + bias.double().abs()) + conv64(e_a, aw)
  return dict(a=a, e_a=e_a, z=z, e_z=e_z, amb=amb, n_amb=n_amb)


# ----------------------------------------------------------------------------- backward layer
def backward_layer(g_a, x, w, z=None, state=None, gamma=None, groups=1, n_lane=16, slope=SLOPE):
  """One backward launch.  MODE 1 (z given): per statistics group g_z = bn_ref.bn_bwd64(g_a, z) with the kernel's own state,
  g_x = g_a + dgrad64(g_z), and per group g_gamma, g_beta.  MODE 0 (conv_alone, z None): g_z = g_a, g_x = dgrad64(g_a), no
  skip term.  dW = wgrad64(x, g_z) and db = sum g_z over ALL groups.

  Model.  g_z is not stored: e_gz = K_BWD U S_gz from bn_ref.bwd_scales with the launch's n_lane (the stage-1 sums the kernel
  merges were taken by lanes of n_lane voxels), plus |gamma| invstd |g_a| (1 - slope) on an ambiguous branch.  MODE 0: 0.
      g_x:  288 products and the skip add, n = 289:   e = gamma(289) (dgrad(|g_z|, |w|) + |g_a|) + dgrad(e_gz, |w|)
      dW :  n = every voxel of the launch:             e = gamma(N) wgrad(|x|, |g_z|) + wgrad(|x|, e_gz)
      db :                                              e = gamma(N) sum|g_z| + sum e_gz
      g_gamma, g_beta: K_BWD U bwd_scales, as tests/test_gpu_batchnorm_fp64.py part C"""
  g_a, x = g_a.double(), x.double()
  B, H, W, _ = g_a.shape
  N = B * H * W
  aw = w.double().abs()
  out = dict(n_amb=0)
  if z is None:
    g_z, e_gz = g_a, torch.zeros_like(g_a)
    res = torch.zeros_like(g_a)
  else:
    per = B // groups
    g_z, e_gz = torch.empty_like(g_a), torch.empty_like(g_a)
    amb = torch.zeros(g_a.shape, dtype=torch.bool)
    gg, gb, e_gg, e_gb = [], [], [], []
    for gi in range(groups):
      sl = slice(gi * per, (gi + 1) * per)
      st = split_state(state, gi)
      ga2, z2 = g_a[sl].reshape(-1, 32), z[sl].reshape(-1, 32)
      ref = br.bn_bwd64(ga2, z2, st, gamma, slope)
      sc = br.bwd_scales(ga2, z2, st, gamma, ref, n_lane, slope)
      e = K_BWD * U * sc["g_z"] + torch.where(ref["amb"], gamma.double().abs() * st["invstd"].double() * ga2.abs() * (1.0 - slope),
                                             torch.zeros_like(ga2))
      g_z[sl] = ref["g_z"].reshape(g_a[sl].shape)
      e_gz[sl] = e.reshape(g_a[sl].shape)
      amb[sl] = ref["amb"].reshape(g_a[sl].shape)
      gg.append(ref["g_gamma"]); gb.append(ref["g_beta"])
      e_gg.append(K_BWD * U * sc["g_gamma"]); e_gb.append(K_BWD * U * sc["g_beta"])
    out.update(g_gamma=torch.stack(gg), g_beta=torch.stack(gb), e_g_gamma=torch.stack(e_gg), e_g_beta=torch.stack(e_gb),
               amb=amb, n_amb=int(amb.sum()))
    res = g_a
  out.update(g_z=g_z, e_gz=e_gz)
  out["g_x"] = res + dgrad64(g_z, w)
  # `own_*`: the summation term alone (what the launch's own additions can err by, given its g_z)
  out["own_g_x"] = gamma_n(289) * (dgrad64(g_z.abs(), aw) + res.abs())
  out["e_g_x"] = out["own_g_x"] + dgrad64(e_gz, aw)
  out["dW"] = wgrad64(x, g_z)
  out["own_dW"] = gamma_n(N) * wgrad64(x.abs(), g_z.abs())
  out["e_dW"] = out["own_dW"] + wgrad64(x.abs(), e_gz)
  out["db"] = g_z.reshape(-1, 32).sum(0)
  out["own_db"] = gamma_n(N) * g_z.abs().reshape(-1, 32).sum(0)
  out["e_db"] = out["own_db"] + e_gz.reshape(-1, 32).sum(0)
  return out


def next_sums(g_x, z_next, state_next, groups=1, n_lane=16, slope=SLOPE):
  """The stage-1 sums a backward launch leaves for the layer below, per group:  sum g_y'  and  sum g_y' (z_next - mean_next),
  g_y' = g_x lrelu'(z_next * scale_next + shift_next), taken from the g_x THE KERNEL STORED (so that the error of g_x does
  not enter).  Model: bn_ref.bwd_scales with the launch's n_lane and K_BWD; an ambiguous branch widens through amb_ga."""
  per = g_x.shape[0] // groups
  ones = torch.ones(32)
  s_dy, s_dx, e_dy, e_dx, n_amb = [], [], [], [], 0
  for gi in range(groups):
    sl = slice(gi * per, (gi + 1) * per)
    st = split_state(state_next, gi)
    gx2, z2 = g_x[sl].reshape(-1, 32), z_next[sl].reshape(-1, 32)
    ref = br.bn_bwd64(gx2, z2, st, ones, slope)
    sc = br.bwd_scales(gx2, z2, st, ones, ref, n_lane, slope)
    s_dy.append(ref["sum_dy"]); s_dx.append(ref["sum_dx"])
    e_dy.append(K_BWD * U * sc["sum_dy"]); e_dx.append(K_BWD * U * sc["sum_dx"])
    n_amb += ref["n_amb"]
  return dict(sum_dy=torch.stack(s_dy), sum_dx=torch.stack(s_dx), e_sum_dy=torch.stack(e_dy), e_sum_dx=torch.stack(e_dx),
              n_amb=n_amb)


# ----------------------------------------------------------------------------- running statistics
def running_update(states, rm, rv, momentum32):
  """as_trunk_finish_fwd's update, group 0 first:  r <- m * batch + (1 - m) * r  per group, in fp64 without intermediate
  rounding, m the fp32 momentum the kernel reads.  states: [groups, 5, 32] of one layer.  The kernel rounds once per update,
  so the bound is one fp32 ulp of the result per update (the first update's error shrinks by 1 - m in the second)."""
  mo = float(torch.tensor(momentum32, dtype=torch.float32))
  m, v = rm.double(), rv.double()
  e_m, e_v = torch.zeros_like(m), torch.zeros_like(v)
  for gi in range(states.shape[0]):
    m = mo * states[gi, 0].double() + (1.0 - mo) * m
    v = mo * states[gi, 4].double() + (1.0 - mo) * v
    e_m = (1.0 - mo) * e_m + br.ulp32(m)
    e_v = (1.0 - mo) * e_v + br.ulp32(v)
  return m, v, e_m, e_v


# ----------------------------------------------------------------------------- the cases the GPU file runs
# (B, H, W, groups, (ph, pw)): the smallest maps at which each index path of the kernels differs
GEOMS = [
  (2, 1, 1, 2, (1, 1)),      # narrower than a tile: the mask cuts both sides of every row
  (2, 3, 5, 2, (2, 2)),
  (2, 2, 31, 2, (1, 3)),     # around the tile width
  (2, 2, 32, 2, (1, 1)),
  (2, 3, 33, 2, (2, 2)),     # shifted last tile, dup = 31
  (2, 9, 44, 2, (1, 3)),     # dup = 20
  (2, 4, 63, 2, (1, 1)),     # dup = 1
  (2, 2, 64, 2, (2, 2)),     # multiples of the tile width
  (2, 3, 65, 2, (1, 3)),
  (2, 24, 78, 2, (1, 1)),    # the KITTI map: 72 tiles, one per workgroup
  (6, 24, 78, 2, (2, 2)),    # 216 tiles in two rounds of 108: a workgroup's second tile lies in another image
  (1, 43, 96, 1, (1, 3)),    # 129 tiles, gper = 65: uneven rounds
  (3, 6, 16, 1, (1, 1)),     # one group of three images
]
BWD_FAMILIES = ["zero_mean", "common_mode", "z_offset", "sent_edges"]
FWD_FAMILIES = ["dense", "positive", "shift_large", "sentinels"]


def geom_id(g):
  return "%dx%dx%d_g%d_h%d%d" % (g[0], g[1], g[2], g[3], g[4][0], g[4][1])


def _gen(seed):
  return torch.Generator().manual_seed(seed)


def chan_scale():
  """different magnitudes per channel, so that a channel swizzle fails"""
  return torch.pow(2.0, (torch.arange(32) % 9 - 4).float())


def case_seed(geom, k=0):
  B, H, W, groups, _ = geom
  return 1000 * k + 7 * B + 131 * H + W


def random_weights(seed, positive=False):
  w = torch.randn(32, 32, 3, 3, generator=_gen(seed)) / 288 ** 0.5
  b = torch.randn(32, generator=_gen(seed + 1)) * 0.1
  return (w.abs(), b.abs()) if positive else (w, b)


# Seeds of the crafted-state cases that had an ambiguous LeakyReLU branch somewhere (with |mean| / std = 1e2 a y within a
# rounding of 0 turns up about once in 1e5 elements) are moved on, here and before any kernel saw them;
# tests/test_trunk_ref_cpu.py asserts that none is left.
BWD_SALT = {("2x24x78_g2_h11", "z_offset"): 3}


def bwd_case(fam, geom):
  """Inputs of a backward MODE 1 launch on crafted states: g_a, z (this layer), x (= a_{l-1}), z_next (the layer below),
  gamma, gamma_next; the two groups get different statistics.  Families: zero-mean g_a; g_a = 50 + noise (k1 matters);
  |mean| / std = 1e2 in z; g_a sentinels of 1e4 at the first voxel, the last voxel of each group, the two columns of the
  shifted tile's seam and the last row."""
  B, H, W, groups, _ = geom
  gen = _gen(case_seed(geom, 1 + BWD_FAMILIES.index(fam)) + BWD_SALT.get((geom_id(geom), fam), 0))
  sc = chan_scale()
  z = torch.randn(B, H, W, 32, generator=gen) * sc
  z_next = torch.randn(B, H, W, 32, generator=gen) * sc
  g_a = torch.randn(B, H, W, 32, generator=gen)
  x = torch.randn(B, H, W, 32, generator=gen)
  per = B // groups
  if groups == 2:
    z[per:] = z[per:] * 1.5 + 0.75 * sc
    z_next[per:] = z_next[per:] * 0.5 - 0.5 * sc
  if fam == "common_mode":
    g_a = g_a + 50.0
  elif fam == "z_offset":
    z = z + 1e2 * sc
    z_next = z_next + 1e2 * sc
  elif fam == "sent_edges":
    seam = tiling(B, H, W, groups)["seam"]
    spots = [(0, 0, 0), (B - 1, H - 1, W - 1), (0, H - 1, W // 2), (0, H // 2, max(seam - 1, 0)), (0, H // 2, seam)]
    spots += [(gi * per + per - 1, H - 1, W - 1) for gi in range(groups)] + [(gi * per, 0, 0) for gi in range(groups)]
    for (b, y, xx) in spots:
      g_a[b, y, xx] = 1e4
  gamma = torch.rand(32, generator=_gen(8)) + 0.5
  gamma_next = torch.rand(32, generator=_gen(18)) + 0.5
  beta = torch.full((32,), CRAFT_BETA)
  return dict(g_a=g_a, z=z, x=x, z_next=z_next, gamma=gamma, gamma_next=gamma_next, beta=beta, beta_next=beta)


def fwd_case(fam, geom):
  """Inputs of a forward MODE 1 launch: src (= z_{l-1}; its partials come from a real MODE 0 launch), skip, gamma, beta,
  weights and bias.  Families: dense zero-mean; all-positive operand and weights (nothing cancels: a dropped tap shows at
  full size); shift large against scale * src (a padded halo that wrongly holds lrelu(shift) + skip moves every border voxel
  far beyond the bound); sentinels of 1e4 in skip at the first and last voxel of each group (both sides of the group
  boundary).  The two groups get different statistics, so that a swapped state fails."""
  B, H, W, groups, _ = geom
  gen = _gen(case_seed(geom, 11 + FWD_FAMILIES.index(fam)))
  sc = chan_scale()
  per = B // groups
  src = torch.randn(B, H, W, 32, generator=gen) * sc
  skip = torch.randn(B, H, W, 32, generator=gen)
  gamma = (torch.rand(32, generator=gen) + 0.5) * (torch.arange(32) % 3 - 1).sign().add(0.5).sign()
  beta = torch.randn(32, generator=gen)
  w, b = random_weights(case_seed(geom, 21), positive=(fam == "positive"))
  if fam == "positive":
    src = torch.rand(B, H, W, 32, generator=gen) * sc            # normalised within +-1.8: |gamma| * 1.8 < beta
    skip = skip.abs()
    gamma, beta = gamma.abs(), torch.full((32,), 4.0)
  elif fam == "shift_large":
    beta = torch.full((32,), 100.0)
  elif fam == "sentinels":
    for gi in range(groups):
      skip[gi * per, 0, 0] = 1e4
      skip[gi * per + per - 1, H - 1, W - 1] = 1e4
  if groups == 2:
    src[per:] = src[per:] * 2.0 + 3.0 * sc
  return dict(src=src, skip=skip, gamma=gamma, beta=beta, w=w, bias=b)
