"""Train-mode BatchNorm against a plain float64 reference (tests/bn_ref.py): the three fp64 merges of (count, mean, M2)
partials on crafted partials (part A), the moment producers against the fp64 moments of the z they stored (part B), and the
backward's sums and stage 3 (part C).  Every bound is K * U * S with U = 2^-24, K fixed per kind of computation and S from
the error model in bn_ref.py; the worst error / bound of every case is reported through conftest.parity_note."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from adaptive_stereo import _native as nat
from adaptive_stereo import hip_ops as ops
from adaptive_stereo.hip_ops import Pcl, ConvShape
import bn_ref as br
from conftest import parity_note

DEV = "cuda:0"
K_MOMENTS = 16           # the producers' moments (part B)
K_BWD = 16               # the backward's sums and stage 3 (part C)
INVSTD_EPS_ONLY = float(torch.tensor(1.0 / math.sqrt(float(torch.tensor(1e-5, dtype=torch.float32))), dtype=torch.float32))


def _gen(seed):
  return torch.Generator().manual_seed(seed)


# ============================================================================= part A: the merges on crafted partials
NPARTS = [1, 7, 31, 32, 33, 257, 4099]
BAD_CH = 5


def _chan_scale():
  """different magnitudes per channel, so that a channel swizzle fails"""
  return torch.pow(2.0, (torch.arange(32) % 9 - 4).double())


def _crafted(kind, P, seed):
  """(cnt [P], mean [P, 32], m2 [P, 32]) float32 partials of one kind"""
  g = _gen(seed)
  sc = _chan_scale()
  cnt = torch.randint(1, 5000, (P,), generator=g).double()
  sd = sc[None, :]
  mean = torch.randn(P, 32, generator=g, dtype=torch.float64) * sd * 0.3 + sc * 2.0
  m2 = cnt[:, None] * sd * sd * (0.5 + torch.rand(P, 32, generator=g, dtype=torch.float64))
  if kind.startswith("empty") and not kind.endswith("_1e5"):
    where = {"empty0": [0], "empty_mid": [P // 2], "empty_end": [P - 1], "empty_all_but_last": list(range(P - 1))}[kind]
    if P == 1 and kind != "empty_all_but_last":
      where = []
    for i in where:
      cnt[i] = 0; mean[i] = 0; m2[i] = 0
  elif kind == "const":
    mean[:] = (1.5 + torch.arange(32).double()) * sc
    m2[:] = 0
  elif kind == "rowconst":
    m2[:] = 0
  elif kind.startswith("offset"):
    ratio = float(kind.split("_")[1])
    mean = mean - sc * 2.0 + ratio * sc * (torch.arange(32) % 2 * 2 - 1).double()
    if kind.endswith("far"):
      mean[0] = mean[0] + 30.0 * sc
  elif kind == "count1":
    cnt[:] = 0; mean[:] = 0; m2[:] = 0
    cnt[P // 2] = 1; mean[P // 2] = sc * 3.0
  elif kind == "count2":
    cnt[:] = 0; mean[:] = 0; m2[:] = 0
    cnt[P - 1] = 1; mean[P - 1] = sc * 3.0
    cnt[P // 2] += 1; mean[P // 2] = sc * 1.0      # (P == 1: a single partial of two values, M2 0 -> mean only)
  elif kind in ("empty0_1e5", "empty0k_1e5"):
    # |mean|/std = 1e5 with partial 0 (and, separately, partials 0 .. P/3) empty: a pivot taken from an empty partial (mean 0)
    # costs (mean/std)^2 = 1e10 in the one-pass cancellation, ~1e-6 relative on the variance, 20x the bound
    mean = mean - sc * 2.0 + 1e5 * sc * (torch.arange(32) % 2 * 2 - 1).double()
    for i in (range(1) if kind == "empty0_1e5" else range(max(1, P // 3))):
      if P > 1:
        cnt[i] = 0; mean[i] = 0; m2[i] = 0
  elif kind == "big":
    cnt = torch.randint(2 ** 23, 2 ** 24 + 1, (P,), generator=g).double()
    m2 = cnt[:, None] * sd * sd * (0.5 + torch.rand(P, 32, generator=g, dtype=torch.float64))
  return cnt.float(), mean.float(), m2.float()


KINDS = ["random", "empty0", "empty_mid", "empty_end", "empty_all_but_last", "const", "rowconst", "offset_1e3_near",
         "offset_1e3_far", "offset_1e4_near", "offset_1e4_far", "offset_1e5_near", "offset_1e5_far", "empty0_1e5", "empty0k_1e5", "count1", "count2", "big"]
BAD = ["nan_m2", "inf_mean", "inf_both"]


def _spoil(cnt, mean, m2, bad):
  mean, m2 = mean.clone(), m2.clone()
  i = cnt.shape[0] // 2
  if bad == "nan_m2":
    m2[i, BAD_CH] = float("nan")
  elif bad == "inf_mean":
    mean[i, BAD_CH] = float("inf")
  else:
    mean[i, BAD_CH] = float("inf"); m2[i, BAD_CH] = float("inf")
  return cnt, mean, m2


def _affine():
  g = _gen(99)
  gamma = (torch.rand(32, generator=g) + 0.5) * (torch.arange(32) % 3 - 1).sign().add(0.5).sign()
  beta = torch.randn(32, generator=g)
  rm, rv = torch.randn(32, generator=g), torch.rand(32, generator=g) + 0.5
  return gamma, beta, rm, rv


class _Merge(object):
  """Runs one of the three merges on partials of two statistics groups (the trunk takes both at once; the others one at a time)
  and returns per group a dict of fp32 results: mean, invstd, scale, shift, and running_mean / running_var (or var_u)."""

  def __init__(self, which):
    self.which = which
    lib = nat.load()
    if which == "agg3d":
      self.g = Pcl(1, 1, 4, 33, 1, 1, 1)
      assert lib.as_agg3d_ok(self.g) == 1
      self.x = ops.pcl_zeros(self.g, DEV)
      self.wp = ops.pack_weights(torch.zeros(32, 32, 3, 3, 3, device=DEV), ops.CONV3D_333, False)
    elif which == "trunk":
      self.g = Pcl(2, 1, 6, 16, 0, 2, 2)
      self.x = ops.pcl_zeros(self.g, DEV)
      self.wp = ops.pack_weights(torch.zeros(32, 32, 3, 3, device=DEV), ops.conv_shape_2d(1), False)
    self.b = torch.zeros(32, device=DEV)

  def run(self, groups, gamma, beta, rm, rv):
    gd, bd = gamma.to(DEV), beta.to(DEV)
    if self.which == "trunk":
      P = groups[0][0].shape[0]
      sp = ops.StatParts(2 * P, DEV)
      sp.cnt.copy_(torch.cat([c for c, _, _ in groups]).to(DEV))
      sp.mean.copy_(torch.cat([m for _, m, _ in groups]).reshape(-1).to(DEV))
      sp.m2.copy_(torch.cat([q for _, _, q in groups]).reshape(-1).to(DEV))
      states = torch.full((2, 5, 32), -7.0, device=DEV)
      bn = nat.TrunkBn(nat.ptr(sp.mean), nat.ptr(sp.m2), nat.ptr(sp.cnt), nat.ptr(gd), nat.ptr(bd), nat.ptr(states), P, 1e-5)
      a_out, z = ops.pcl_zeros(self.g, DEV), ops.pcl_zeros(self.g, DEV)
      nat.call("as_trunk_fwd", nat.ptr(self.x), nat.ptr(self.x), bn, nat.ptr(a_out), self.g, 2, nat.ptr(self.wp), nat.ptr(self.b),
               0.2, nat.ptr(z), None, None, None, nat.stream())
      s = states.cpu().double()
      return [dict(mean=s[i, 0], invstd=s[i, 1], scale=s[i, 2], shift=s[i, 3], var_u=s[i, 4]) for i in range(2)]
    out = []
    for cnt, mean, m2 in groups:
      sp = ops.StatParts(cnt.shape[0], DEV)
      sp.cnt.copy_(cnt.to(DEV)); sp.mean.copy_(mean.reshape(-1).to(DEV)); sp.m2.copy_(m2.reshape(-1).to(DEV))
      rm_d, rv_d = rm.to(DEV).clone(), rv.to(DEV).clone()
      if self.which == "finalize":
        st = ops.bn_train_stats(sp, gd, bd, rm_d, rv_d)
      else:
        pend = ops.PendingBn(sp, gd, bd, rm_d, rv_d)
        ops.agg3d(self.x, self.g, self.wp, self.b, z=ops.pcl_zeros(self.g, DEV), in_bn=pend, a_out=ops.pcl_zeros(self.g, DEV))
        st = pend.state
      out.append(dict(mean=st.mean.cpu().double(), invstd=st.invstd.cpu().double(), scale=st.scale.cpu().double(),
                      shift=st.shift.cpu().double(), running_mean=rm_d.cpu().double(), running_var=rv_d.cpu().double()))
    return out


@pytest.mark.parametrize("nparts", NPARTS)
@pytest.mark.parametrize("which", ["finalize", "agg3d", "trunk"])
def test_merge_of_crafted_partials_against_fp64(which, nparts):
  """as_bn_finalize, the consumer merge of as_agg3d_fwd (bn_merge.h) and the trunk's per-group merge, on crafted fp32 partials:
  empty partials (at index 0 too), constant channels (bit-exact), M2 = 0 with different means, |mean|/std up to 1e5 with
  partial 0 near and far, total counts of 1 and 2, counts up to 2^24, per-channel magnitudes; fp64 arithmetic rounded once,
  so the bound is 1 ulp plus the fp64 cancellation of the one-pass form (bn_ref.merge_bounds)."""
  m = _Merge(which)
  gamma, beta, rm, rv = _affine()
  worst = {}
  kinds = KINDS
  for ki in range(0, len(kinds), 2):
    pair = [_crafted(k, nparts, seed=nparts * 100 + ki + j) for j, k in enumerate(kinds[ki:ki + 2])]
    if len(pair) == 1:
      pair.append(_crafted("random", nparts, seed=7))
    got = m.run(pair, gamma, beta, rm, rv)
    for j, (cnt, mean, m2) in enumerate(pair):
      kind = kinds[ki + j] if ki + j < len(kinds) else "random"
      tag = "%s P%d %s" % (which, nparts, kind)
      n, mu, q = br.chan_merge64(cnt, mean, m2)
      ref = br.bn_state64(n, mu, q, gamma, beta, rm, rv)
      bnd = br.merge_bounds(cnt, mean, m2, gamma, ref, c=nparts + 32)
      fields = ["mean", "invstd", "scale", "shift"] + (["var_u"] if which == "trunk" else ["running_mean", "running_var"])
      for f in fields:
        err = (got[j][f] - ref[f]).abs()
        r = br.worst_ratio(err, bnd[f])
        worst[f] = max(worst.get(f, 0.0), r)
        assert r <= 1.0, "%s: %s err/bound %.3g (err %.3e)" % (tag, f, r, float(err.max()))
      if kind == "const":
        assert torch.equal(got[j]["mean"].float(), mean[0]), tag + ": the mean of a constant channel must be exact"
        assert bool((got[j]["invstd"].float() == INVSTD_EPS_ONLY).all()), tag + ": invstd of a constant channel"
  # non-finite partials: that channel NaN as torch gives, the other 31 bit-identical to the clean run
  clean = _crafted("random", nparts, seed=5)
  base = m.run([clean, clean], gamma, beta, rm, rv)[0]
  for bad in BAD:
    res = m.run([_spoil(*clean, bad), clean], gamma, beta, rm, rv)
    spoilt, other = res[0], res[1]
    tag = "%s P%d %s" % (which, nparts, bad)
    vfield = "var_u" if which == "trunk" else "running_var"
    assert bool(torch.isnan(spoilt["invstd"][BAD_CH])), tag + ": invstd %r, torch gives NaN" % float(spoilt["invstd"][BAD_CH])
    assert bool(torch.isnan(spoilt[vfield][BAD_CH])), tag + ": %s %r, torch gives NaN" % (vfield, float(spoilt[vfield][BAD_CH]))
    keep = torch.arange(32) != BAD_CH
    for f in base:
      assert torch.equal(spoilt[f][keep], base[f][keep]), tag + ": channel %s changed in the other channels" % f
      assert torch.equal(other[f], base[f]), tag + ": the other group changed"
  parity_note("bn_merge[%s P%d]" % (which, nparts), **{"worst_err_over_bound_" + f: v for f, v in worst.items()})


# ============================================================================= part B: the moment producers
def _identity_weights(kd):
  w = torch.zeros(32, 32, 3, 3, 3) if kd > 1 else torch.zeros(32, 32, 3, 3)
  idx = torch.arange(32)
  if kd > 1:
    w[idx, idx, 1, 1, 1] = 1.0
  else:
    w[idx, idx, 1, 1] = 1.0
  return w


def _family_input(fam, B, D, H, W, seed, positive=False):
  """x [B, D, H, W, 32] (channel last, the PCL interior) and the bias of a data family; with identity weights z = x + b.
  Returns (x, bias, const_channels, sentinel_index or None)."""
  g = _gen(seed)
  x = torch.randn(B, D, H, W, 32, generator=g)
  sc = _chan_scale().float()
  x = x * sc
  bias = torch.randn(32, generator=g) * 0.1
  const = []
  sent = None
  if positive:                              # operands that pass through the LeakyReLU unchanged
    x = x.abs() + 0.01
  if fam == "offsets":
    off = 1e3 * sc * (torch.arange(32) % 2 * 2 - 1).float()
    x = x + (off.abs() if positive else off)
  elif fam == "pivot_far":
    x[:, :, :, ::128, :] += 100.0 * sc
    x[:, :, :, ::32, :] += 100.0 * sc       # (the first voxel of a 32-voxel tile as well)
  elif fam == "const":
    const = list(range(0, 32, 4))
    x[..., const] = 0.0
    bias[const] = torch.arange(len(const)).float() * 0.25 + 0.5      # dyadic: a sum of copies and its quotient are exact
  elif fam.startswith("sent_"):
    where = fam[5:]
    b, d, y, xx = {"tail": (0, D - 1, H // 2, W - 1), "dup": (0, 0, H // 2, W - 127 if W > 128 else W // 2),
                   "dup64": (0, 0, H // 2, W - 63 if W > 64 else W // 2), "first_row": (0, 0, 0, W // 3),
                   "last_row": (0, D - 1, H - 1, W // 2), "last_image": (B - 1, D // 2, H // 2, W // 2),
                   "first_plane": (0, 0, H // 2, W // 2), "last_plane": (B - 1, D - 1, H // 2, W // 3),
                   "group_edge": (B // 2, 0, 0, 0)}[where]
    x[b, d, y, xx, :] = 1e4 * sc
    sent = (b, d, y, xx)
  return x, bias, const, sent


def check_producer(tag, z, stats, merges, const=(), sent=None, groups=1):
  """The producer's partials (stats) against the fp64 moments of the z [..., 32] it stored; also through as_bn_finalize.
  `sent`: the statistics group that holds a sentinel (the bound must be far below what dropping it would move)."""
  z = z.reshape(-1, 32)
  N = z.shape[0]
  cnt, mean, m2 = stats.cnt.double(), stats.mean.view(-1, 32).double(), stats.m2.view(-1, 32).double()
  P = cnt.shape[0] // groups
  assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(m2).all()) and bool(torch.isfinite(cnt).all()), \
      tag + ": a partial slot the merge reads is not finite"
  assert bool((cnt == cnt.round()).all()) and bool((cnt >= 0).all()), tag + ": counts must be whole numbers"
  ratios = {}
  zg = z.view(groups, -1, 32)
  for gi in range(groups):
    c_g, mu_g, q_g = cnt[gi * P:(gi + 1) * P], mean[gi * P:(gi + 1) * P], m2[gi * P:(gi + 1) * P]
    Ng = zg.shape[1]
    assert float(c_g.sum()) == float(Ng), tag + ": sum of counts %r != %d" % (float(c_g.sum()), Ng)
    n64, mu64, q64 = br.moments64(zg[gi])
    # lane model: every producer here folds 8 (wave, half) lanes per channel into its partial, and a tile (row segment, unit,
    # plane run) gives each lane the same share — 16 voxels of a 128-voxel tile — except a ragged / shifted-back tile, which
    # gives fewer: a lane holds at most cnt/8 + one tile's share.  (The tile-epilogue producers, conv3d and the trunk, sum a
    # tile in two passes and fold tiles with `merges` fp32 Chan steps: their lanes are shorter than this.)
    n_lane = math.ceil(float(c_g.max()) / 8) + 16
    s_mean, s_var = br.producer_scales(zg[gi], n_lane, 8 * P, merges)
    nk, muk, qk = br.chan_merge64(c_g, mu_g, q_g)
    e_mean = (muk - mu64).abs()
    e_var = (qk / nk - q64 / Ng).abs()
    r_m = br.worst_ratio(e_mean, K_MOMENTS * br.U * s_mean)
    r_v = br.worst_ratio(e_var, K_MOMENTS * br.U * s_var)
    ratios["mean_g%d" % gi] = r_m; ratios["var_g%d" % gi] = r_v
    assert r_m <= 1.0, "%s group %d: mean err/bound %.3g (err %.3e)" % (tag, gi, r_m, float(e_mean.max()))
    assert r_v <= 1.0, "%s group %d: var err/bound %.3g (err %.3e)" % (tag, gi, r_v, float(e_var.max()))
    for c in const:
      live = c_g > 0
      v = zg[gi, 0, c]
      assert bool((zg[gi, :, c] == v).all()), tag + ": channel %d is not constant in z" % c
      assert bool((mu_g[live, c] == float(v)).all()) and bool((q_g[live, c] == 0).all()), \
          tag + ": constant channel %d: partials mean/M2 not exact" % c
    if sent == gi:
      # teeth: dropping the sentinel or counting it twice moves the mean by |z_s - mean| / N
      shift = (zg[gi].double() - mu64).abs().max(0).values / Ng
      assert bool((K_MOMENTS * br.U * s_mean < 0.1 * shift).all()), tag + ": the bound cannot see the sentinel"
  if groups == 1:
    gam, bet = torch.ones(32, device=z.device), torch.zeros(32, device=z.device)
    rm, rv = torch.zeros(32, device=z.device), torch.ones(32, device=z.device)
    st = ops.bn_train_stats(stats, gam, bet, rm, rv)
    n64, mu64, q64 = br.moments64(z)
    e_mean = (st.mean.double() - mu64).abs()
    var64 = q64 / N
    inv64 = 1.0 / torch.sqrt(var64 + br.EPS)
    e_inv = (st.invstd.double() - inv64).abs()
    b_inv = 0.5 * inv64 ** 3 * K_MOMENTS * br.U * s_var + br.ulp32(inv64)
    r_fm = br.worst_ratio(e_mean, K_MOMENTS * br.U * s_mean + br.ulp32(mu64))
    r_fi = br.worst_ratio(e_inv, b_inv)
    ratios["finalize_mean"] = r_fm; ratios["finalize_invstd"] = r_fi
    assert r_fm <= 1.0 and r_fi <= 1.0, "%s: through as_bn_finalize: mean %.3g invstd %.3g of the bound" % (tag, r_fm, r_fi)
    for c in const:
      assert float(st.mean[c]) == float(z[0, c]) and float(st.invstd[c]) == INVSTD_EPS_ONLY, tag + ": constant channel %d" % c
  parity_note("bn_moments[%s]" % tag, n_lane=int(math.ceil(float(cnt.max()) / 8) + 16),
              **{"worst_err_over_bound_" + k: v for k, v in ratios.items()})


FAMILIES = ["zero_mean", "offsets", "pivot_far", "const"]


def _run_conv32(fam, B, D, H, W, shape, halo, seed=1, random_w=False):
  g = Pcl(B, D, H, W, *halo)
  x, bias, const, sent = _family_input(fam, B, D, H, W, seed)
  if random_w:
    w = torch.randn(*((32, 32, 3, 3, 3) if shape.kd > 1 else (32, 32, 3, 3)), generator=_gen(3)) / (32 * shape.taps()) ** 0.5
  else:
    w = _identity_weights(shape.kd)
  xb = ops.pcl_zeros(g, DEV)
  ops.pcl_interior(xb, g).copy_(x.to(DEV))
  stats = ops.conv32_stat_parts(g, g, shape, DEV)
  z = ops.conv32(xb, g, ops.pack_weights(w.to(DEV), shape, False), bias.to(DEV), g, shape, out=ops.pcl_zeros(g, DEV), stats=stats)
  return ops.pcl_interior(z, g).contiguous(), stats, const, sent


CONV_GEOMS = [  # B, D, H, W, shape, halo: 3-D tile-epilogue / LDS instances, 2-D LDS with ragged tails and dilations
  (2, 12, 6, 19, ConvShape(3, 3, 3, 1, 1, 1, 1, 1), (1, 1, 1)),
  (1, 5, 9, 40, ConvShape(3, 3, 3, 1, 1, 1, 1, 1), (1, 1, 1)),
  (2, 1, 4, 33, ConvShape(3, 3, 3, 1, 1, 1, 1, 1), (1, 1, 1)),
  (2, 1, 17, 37, ConvShape(1, 3, 3, 0, 1, 1, 1, 1), (0, 1, 1)),
  (2, 1, 19, 300, ConvShape(1, 3, 3, 0, 1, 1, 1, 1), (0, 8, 8)),
  (1, 1, 23, 257, ConvShape(1, 3, 3, 0, 4, 4, 4, 1), (0, 8, 8)),
  (1, 1, 375, 1242, ConvShape(1, 3, 3, 0, 2, 2, 2, 1), (0, 8, 8)),
]


@pytest.mark.parametrize("B,D,H,W,shape,halo", CONV_GEOMS)
def test_conv32_fwd_moments(B, D, H, W, shape, halo):
  """as_conv32_fwd's partials (tile epilogue and LDS instances) against the fp64 moments of its z: every data family, the
  sentinels at the edges of small geometries, one random-weight case"""
  small = B * D * H * W <= 12000
  fams = FAMILIES + (["sent_tail", "sent_dup", "sent_first_row", "sent_last_row", "sent_last_image"] if small else [])
  merges = math.ceil(B * D * H * W / nat.load().as_conv32_stat_parts(Pcl(B, D, H, W, *halo), Pcl(B, D, H, W, *halo), shape) / 32) + 8
  for fam in fams:
    z, stats, const, sent = _run_conv32(fam, B, D, H, W, shape, halo)
    check_producer("conv32 %s B%d D%d H%d W%d d%d" % (fam, B, D, H, W, shape.dil), z, stats, merges, const,
                   0 if sent else None)
  z, stats, _, _ = _run_conv32("zero_mean", B, D, H, W, shape, halo, random_w=True)
  check_producer("conv32 random_w B%d D%d H%d W%d d%d" % (B, D, H, W, shape.dil), z, stats, merges)


def _run_act(kind, fam, B, H, W, dil, seed=1, random_w=False):
  """as_conv32_act_fwd / as_conv32_wino_fwd with scale 1, shift 0 and positive operands: a_prev = z_prev, z = a_prev + b"""
  g = Pcl(B, 1, H, W, 0, 8, 8)
  shape = ops.conv_shape_2d(dil)
  lib = nat.load()
  x, bias, const, sent = _family_input(fam, B, 1, H, W, seed, positive=True)
  w = (torch.randn(32, 32, 3, 3, generator=_gen(3)) * 0.06) if random_w else _identity_weights(1)
  w = w.to(DEV)
  zp = ops.pcl_zeros(g, DEV)
  ops.pcl_interior(zp, g).copy_(x.to(DEV))
  st = ops.BnState(DEV)
  st.scale.fill_(1.0); st.shift.fill_(0.0)
  a_out, z = ops.pcl_zeros(g, DEV), ops.pcl_zeros(g, DEV)
  bd = bias.to(DEV)
  if kind == "wino":
    assert lib.as_conv32_wino_ok(g, g, shape) == 1
    ww = torch.empty(16 * 1024, device=DEV)
    nat.call("as_conv32_wino_pack_weights", nat.ptr(w), nat.ptr(ww), 0, nat.stream())
    stats = ops.StatParts(lib.as_conv32_wino_parts(), DEV)
    nat.call("as_conv32_wino_fwd", nat.ptr(zp), None, nat.ptr(st.scale), nat.ptr(st.shift), nat.ptr(a_out), g, nat.ptr(ww),
             nat.ptr(bd), 0.2, nat.ptr(z), g, shape, nat.ptr(stats.mean), nat.ptr(stats.m2), nat.ptr(stats.cnt), nat.stream())
  else:
    assert lib.as_conv32_act_ok(g, g, shape) == 1
    wp = ops.pack_weights(w, shape, False)
    stats = ops.StatParts(lib.as_conv32_act_parts(), DEV)
    nat.call("as_conv32_act_fwd", nat.ptr(zp), None, nat.ptr(st.scale), nat.ptr(st.shift), nat.ptr(a_out), g, nat.ptr(wp),
             nat.ptr(bd), 0.2, nat.ptr(z), g, shape, nat.ptr(stats.mean), nat.ptr(stats.m2), nat.ptr(stats.cnt), nat.stream())
  return ops.pcl_interior(z, g).contiguous(), stats, const, sent


# (the smallest launches these kernels take have 4 tiles per workgroup: (2, 520, 262) is near that floor)
ACT_GEOMS = [(2, 161, 1242, 2), (4, 97, 700, 1), (2, 163, 1237, 8), (2, 520, 262, 1), (4, 375, 1242, 1)]


@pytest.mark.parametrize("kind", ["act", "wino"])
@pytest.mark.parametrize("B,H,W,dil", ACT_GEOMS)
def test_refinement_producers_moments(kind, B, H, W, dil):
  """as_conv32_act_fwd and as_conv32_wino_fwd (the refinement's production route) against the fp64 moments of their z, the
  bench shape at 4 pairs included; sentinels on the small geometry"""
  small = B * H * W <= 300000
  fams = ["zero_mean", "offsets", "pivot_far", "const"] + (["sent_tail", "sent_dup", "sent_dup64", "sent_first_row", "sent_last_row",
                                                   "sent_last_image"] if small else [])
  for fam in fams:
    z, stats, const, sent = _run_act(kind, fam, B, H, W, dil)
    check_producer("%s %s B%d H%d W%d d%d" % (kind, fam, B, H, W, dil), z, stats, 8, const, 0 if sent else None)
  z, stats, _, _ = _run_act(kind, "zero_mean", B, H, W, dil, random_w=True)
  check_producer("%s random_w B%d H%d W%d d%d" % (kind, B, H, W, dil), z, stats, 8)


def test_wino_moments_at_32_pairs():
  """the refinement at 32 pairs (B = 32, 375 x 1242) through the wino forward: the largest per-lane count the bench runs"""
  for fam in ("zero_mean", "offsets"):
    z, stats, _, _ = _run_act("wino", fam, 32, 375, 1242, 1)
    check_producer("wino %s B32 H375 W1242 d1" % fam, z, stats, 8)
    del z, stats
    torch.cuda.empty_cache()


AGG_GEOMS = [(1, 12, 24, 78), (3, 5, 9, 40), (1, 1, 4, 33), (2, 7, 6, 81), (4, 12, 24, 78),
             (1, 2, 3, 120), (1, 2, 2, 156)]      # column strips: the second right-aligned over 4 overlap columns; no overlap


@pytest.mark.parametrize("B,D,H,W", AGG_GEOMS)
def test_agg3d_moments(B, D, H, W):
  """as_agg3d_fwd: layer 1 (raw operand) in every family and with random weights, sentinels on the first / last plane and the
  other edges; layers 2-4 (the fused operand: the previous layer's partials merged in the kernel and applied with the
  LeakyReLU while staging)"""
  g = Pcl(B, D, H, W, 1, 1, 1)
  lib = nat.load()
  assert lib.as_agg3d_ok(g) == 1
  wp = ops.pack_weights(_identity_weights(3).to(DEV), ops.CONV3D_333, False)
  nparts = lib.as_agg3d_parts(g)
  fams = FAMILIES + ["sent_first_plane", "sent_last_plane", "sent_tail", "sent_first_row", "sent_last_row", "sent_last_image"]
  for fam in fams:
    x, bias, const, sent = _family_input(fam, B, D, H, W, seed=2)
    xb = ops.pcl_zeros(g, DEV)
    ops.pcl_interior(xb, g).copy_(x.to(DEV))
    stats = ops.StatParts(nparts, DEV)
    z = ops.agg3d(xb, g, wp, bias.to(DEV), z=ops.pcl_zeros(g, DEV), stats=stats)
    if sent is not None and B * D * H * W > 12000:
      sent = None
    check_producer("agg3d L1 %s B%d D%d H%d W%d" % (fam, B, D, H, W), ops.pcl_interior(z, g).contiguous(), stats, 8, const,
                   0 if sent else None)
  wr = torch.randn(32, 32, 3, 3, 3, generator=_gen(3)) / 864 ** 0.5
  wpr = ops.pack_weights(wr.to(DEV), ops.CONV3D_333, False)
  x, bias, _, _ = _family_input("offsets", B, D, H, W, seed=4)
  xb = ops.pcl_zeros(g, DEV)
  ops.pcl_interior(xb, g).copy_(x.to(DEV))
  stats = ops.StatParts(nparts, DEV)
  z = ops.agg3d(xb, g, wpr, bias.to(DEV), z=ops.pcl_zeros(g, DEV), stats=stats)
  check_producer("agg3d L1 random_w B%d D%d H%d W%d" % (B, D, H, W), ops.pcl_interior(z, g).contiguous(), stats, 8)
  # layers 2-4: each consumes the partials of the layer before (gamma 1, beta 0: the operand is the normalised z of that layer,
  # through both LeakyReLU branches), with identity weights for layer 2 and random weights after
  keep = []
  for layer, wl in ((2, wp), (3, wpr), (4, wpr)):
    pend = ops.PendingBn(stats, torch.ones(32, device=DEV), torch.zeros(32, device=DEV), torch.zeros(32, device=DEV),
                         torch.ones(32, device=DEV))
    keep.append((z, pend))
    stats = ops.StatParts(nparts, DEV)
    z = ops.agg3d(z, g, wl, bias.to(DEV), z=ops.pcl_zeros(g, DEV), in_bn=pend, a_out=ops.pcl_zeros(g, DEV), stats=stats)
    check_producer("agg3d L%d fused B%d D%d H%d W%d" % (layer, B, D, H, W), ops.pcl_interior(z, g).contiguous(), stats, 8)


@pytest.mark.parametrize("B,H,W", [(1, 21, 30), (2, 75, 131), (8, 375, 1242)])
def test_conv4_moments(B, H, W):
  """as_conv4_fwd's moments (the head's first layer: 3 channels, 5 x 5, stride 2) against fp64: random weights, then an
  input with a large common offset"""
  lib = nat.load()
  shape = ConvShape(1, 5, 5, 0, 2, 2, 1, 2)
  Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
  g4, gout = Pcl(B, 1, H, W, 0, 2, 2), Pcl(B, 1, Ho, Wo, 0, 2, 2)
  for tag, offset in (("plain", 0.0), ("offsets", 300.0)):
    x = torch.randn(B, 3, H, W, generator=_gen(1)) + offset
    w = torch.randn(32, 3, 5, 5, generator=_gen(2)) / 75 ** 0.5
    b = torch.randn(32, generator=_gen(3)) * 0.1
    x4 = torch.zeros(lib.as_pcl4_numel(g4), device=DEV)
    xd = x.to(DEV)
    nat.call("as_pack_in4", None, nat.ptr(xd), 3, nat.ptr(x4), g4, nat.stream())
    wd, bd = w.to(DEV), b.to(DEV)
    wp = torch.empty(25 * 128, device=DEV)
    nat.call("as_conv4_pack_weights", nat.ptr(wd), 3, nat.ptr(wp), shape, nat.stream())
    nparts = lib.as_conv4_stat_parts(g4, gout, shape)
    stats = ops.StatParts(nparts, DEV)
    z = ops.pcl_zeros(gout, DEV)
    nat.call("as_conv4_fwd", nat.ptr(x4), g4, nat.ptr(wp), nat.ptr(bd), nat.ptr(z), gout, shape, 0, None, None, 0.2,
             nat.ptr(stats.mean), nat.ptr(stats.m2), nat.ptr(stats.cnt), nat.stream())
    merges = math.ceil(B * Ho * Wo / nparts / 32) + 8
    assert int(stats.cnt.sum()) == B * Ho * Wo
    check_producer("conv4 %s B%d H%d W%d" % (tag, B, H, W), ops.pcl_interior(z, gout).contiguous(), stats, merges)


@pytest.mark.parametrize("B,H,W", [(2, 6, 16), (2, 24, 78), (8, 24, 78)])
def test_trunk_moments_per_group(B, H, W):
  """as_trunk_fwd (first layer, two statistics groups): moments per group against fp64, a sentinel on the group boundary"""
  g = Pcl(B, 1, H, W, 0, 2, 2)
  lib = nat.load()
  parts = lib.as_trunk_parts(g, 2)
  wp = ops.pack_weights(_identity_weights(1).to(DEV), ops.conv_shape_2d(1), False)
  wpr = ops.pack_weights((torch.randn(32, 32, 3, 3, generator=_gen(3)) / 288 ** 0.5).to(DEV), ops.conv_shape_2d(1), False)
  for fam in ("zero_mean", "offsets", "pivot_far", "const", "sent_group_edge", "random_w"):
    x, bias, const, sent = _family_input("zero_mean" if fam == "random_w" else fam, B, 1, H, W, seed=6)
    if fam == "offsets":                     # the two groups far apart as well
      x[B // 2:] += 50.0
    xb = ops.pcl_zeros(g, DEV)
    ops.pcl_interior(xb, g).copy_(x.to(DEV))
    stats = ops.StatParts(2 * parts, DEV)
    z = ops.pcl_zeros(g, DEV)
    nat.call("as_trunk_fwd", nat.ptr(xb), None, None, None, g, 2, nat.ptr(wpr if fam == "random_w" else wp), nat.ptr(bias.to(DEV)),
             0.2, nat.ptr(z),
             nat.ptr(stats.mean), nat.ptr(stats.m2), nat.ptr(stats.cnt), nat.stream())
    merges = math.ceil(B * H * W / 2 / parts / 32) + 8
    check_producer("trunk %s B%d H%d W%d" % (fam, B, H, W), ops.pcl_interior(z, g).contiguous(), stats, merges, const,
                   1 if sent else None, groups=2)


# ============================================================================= part C: the backward
def _bwd_lane(g):
  nch = g.B * g.D * g.H * ((g.W + 127) // 128)
  nb = min(1024, max(1, (nch + 3) // 4))
  return 4 * math.ceil((((nch + 7) >> 3) << 3) / nb)


def _bwd_inputs(fam, B, H, W, seed):
  gen = _gen(seed)
  z = torch.randn(B, 1, H, W, 32, generator=gen) * _chan_scale().float()
  g_a = torch.randn(B, 1, H, W, 32, generator=gen)
  if fam == "common_mode":
    g_a = g_a + 50.0
  elif fam == "z_offset":
    z = z + 1e2 * _chan_scale().float()
  elif fam == "sent_edges":       # first row, last voxel of the batch, the shifted-back last tile (128) / unit (64), ragged tail
    for (b, y, x) in ((0, 0, W // 3), (B - 1, H - 1, W - 1), (B // 2, H // 2, W - 2), (0, H // 2, W - 127), (B - 1, 1, W - 63)):
      g_a[b, 0, y, x] = 1e4
  return z, g_a


@pytest.mark.parametrize("B,H,W", [(2, 19, 300), (4, 375, 1242), (32, 375, 1242)])
def test_bn_act_bwd_against_fp64(B, H, W):
  """as_bn_act_bwd (stages 1-3) against bn_bwd64 with the state the kernel used: g_gamma, g_beta (stage-1 sums) and g_z"""
  g = Pcl(B, 1, H, W, 0, 8, 8)
  n_lane = _bwd_lane(g)
  gamma = (torch.rand(32, generator=_gen(8)) + 0.5)
  fams = ["zero_mean", "common_mode", "z_offset"] + (["sent_edges"] if B * H * W <= 12000 else [])
  for fam in fams:
    z, g_a = _bwd_inputs(fam, B, H, W, seed=B + H)
    zd, gad = z.to(DEV), g_a.to(DEV)
    z64 = zd.reshape(-1, 32).double()
    st = ops.BnState(DEV)
    st.mean.copy_(z64.mean(0).float())
    st.invstd.copy_((1.0 / torch.sqrt(z64.var(0, unbiased=False) + br.EPS)).float())
    gd = gamma.to(DEV)
    st.scale.copy_(st.invstd * gd); st.shift.copy_(-st.mean * st.scale)
    zb, gab = ops.pcl_zeros(g, DEV), ops.pcl_zeros(g, DEV)
    ops.pcl_interior(zb, g).copy_(zd); ops.pcl_interior(gab, g).copy_(gad)
    g_z, g_gamma, g_beta = ops.bn_act_bwd(gab, zb, st, gd, g, True)
    state = dict(mean=st.mean.clone(), invstd=st.invstd.clone(), scale=st.scale.clone(), shift=st.shift.clone())
    ref = br.bn_bwd64(gad.reshape(-1, 32), zd.reshape(-1, 32), state, gd)
    sc = br.bwd_scales(gad.reshape(-1, 32), zd.reshape(-1, 32), state, gd, ref, n_lane)
    tag = "bn_act_bwd %s B%d H%d W%d" % (fam, B, H, W)
    ratios = {}
    for name, got in (("g_gamma", g_gamma), ("g_beta", g_beta)):
      r = br.worst_ratio((got.double() - ref[name]).abs(), K_BWD * br.U * sc[name])
      ratios[name] = r
      assert r <= 1.0, "%s: %s err/bound %.3g" % (tag, name, r)
    gz = ops.pcl_interior(g_z, g).reshape(-1, 32).double()
    bound = K_BWD * br.U * sc["g_z"]
    if ref["n_amb"]:
      bound = bound + torch.where(ref["amb"], gd.double().abs() * state["invstd"].double() * gad.reshape(-1, 32).double().abs(),
                                  torch.zeros_like(bound))
    r = br.worst_ratio((gz - ref["g_z"]).abs(), bound)
    ratios["g_z"] = r
    assert r <= 1.0, "%s: g_z err/bound %.3g" % (tag, r)
    parity_note("bn_bwd[%s]" % tag, n_lane=n_lane, ambiguous_branches=ref["n_amb"],
                **{"worst_err_over_bound_" + k: v for k, v in ratios.items()})
    del zb, gab, g_z


def _state64(z, gamma):
  """a BatchNorm state [mean, invstd, scale, shift] from z's fp64 moments, rounded to fp32 (what a finalize gives)"""
  z64 = z.reshape(-1, 32).double()
  st = ops.BnState(DEV)
  st.mean.copy_(z64.mean(0).float())
  st.invstd.copy_((1.0 / torch.sqrt(z64.var(0, unbiased=False) + br.EPS)).float())
  st.scale.copy_(st.invstd * gamma); st.shift.copy_(-st.mean * st.scale)
  return st, dict(mean=st.mean.clone(), invstd=st.invstd.clone(), scale=st.scale.clone(), shift=st.shift.clone())


def _check_bwd(tag, ratios, name, got, exp, bound):
  r = br.worst_ratio((got.double() - exp).abs(), bound)
  ratios[name] = max(ratios.get(name, 0.0), r)
  assert r <= 1.0, "%s: %s err/bound %.3g" % (tag, name, r)


@pytest.mark.parametrize("B,H,W,dil", [(2, 520, 262, 1), (4, 375, 1242, 1), (2, 163, 1237, 8)])
def test_fused_backward_paths_against_fp64(B, H, W, dil):
  """The refinement layer's production backward, both routes, against bn_bwd64:
  - stage 3 g_z from as_conv32_wgrad_bnapply (direct) and as_conv32_wino_bwd (minimal filtering), on the coefficients of
    as_bn_act_bwd (stage-1 lane model _bwd_lane);
  - the next layer's stage-1 sums fused into the data gradient, as_conv32_fwd_bnbwd (conv32_lds: 8 (wave, half) lanes per
    channel, 16 voxels of every 128-voxel tile each, dup rows of the shifted-back tile skipped) and as_conv32_wino_bwd (every
    lane bounded by its workgroup's whole share of 128-voxel units), read through as_bn_act_bwd_given: g_gamma, g_beta and
    stage 3, against bn_bwd64 of the g_x each route stored.
  Families: zero-mean g_a, g_a = 50 + noise, |mean|/std = 1e2 in z, g_a sentinels at the edges (small geometry)."""
  g = Pcl(B, 1, H, W, 0, 8, 8)
  shape = ops.conv_shape_2d(dil)
  lib = nat.load()
  assert lib.as_conv32_wino_ok(g, g, shape) == 1 and lib.as_conv32_bnbwd_parts(g, g, shape) > 0
  N = B * H * W
  tiles = B * H * ((W + 127) // 128)
  lane_lds = 16 * math.ceil(tiles / lib.as_conv32_bnbwd_parts(g, g, shape)) + 16
  units = B * ((W + 63) // 64) * sum(((H - r + dil - 1) // dil + 1) // 2 for r in range(dil))
  lane_wino = 128 * math.ceil(units / lib.as_conv32_wino_bwd_parts())
  w = (torch.randn(32, 32, 3, 3, generator=_gen(9)) * 0.06).to(DEV)
  wp_t = ops.pack_weights(w, shape, True)
  ww_t = torch.empty(16 * 1024, device=DEV)
  nat.call("as_conv32_wino_pack_weights", nat.ptr(w), nat.ptr(ww_t), 1, nat.stream())
  gamma = (torch.rand(32, generator=_gen(8)) + 0.5).to(DEV)
  gamman = (torch.rand(32, generator=_gen(18)) + 0.5).to(DEV)
  x = ops.pcl_zeros(g, DEV)
  ops.pcl_interior(x, g).copy_(torch.randn(B, 1, H, W, 32, generator=_gen(7)).to(DEV))
  fams = ["zero_mean", "common_mode", "z_offset"] + (["sent_edges"] if N <= 300000 else [])
  for fam in fams:
    tag = "fused bwd %s B%d H%d W%d d%d" % (fam, B, H, W, dil)
    z, g_a = _bwd_inputs(fam, B, H, W, seed=B + H)
    zn, _ = _bwd_inputs("z_offset" if fam == "z_offset" else "zero_mean", B, H, W, seed=B + H + 1)
    zd, gad, znd = z.to(DEV), g_a.to(DEV), zn.to(DEV)
    st, state = _state64(zd, gamma)
    stn, staten = _state64(znd, gamman)
    zb, gab, znb = ops.pcl_zeros(g, DEV), ops.pcl_zeros(g, DEV), ops.pcl_zeros(g, DEV)
    ops.pcl_interior(zb, g).copy_(zd); ops.pcl_interior(gab, g).copy_(gad); ops.pcl_interior(znb, g).copy_(znd)
    ws = torch.empty(lib.as_bn_bwd_workspace(g), device=DEV)
    gg, gb = torch.zeros(32, device=DEV), torch.zeros(32, device=DEV)
    nat.call("as_bn_act_bwd", nat.ptr(gab), nat.ptr(zb), nat.ptr(st.scale), nat.ptr(st.shift), nat.ptr(st.mean),
             nat.ptr(st.invstd), nat.ptr(gamma), 0.2, 1, None, nat.ptr(gg), nat.ptr(gb), 0, nat.ptr(ws), g, nat.stream())
    coef = ws[lib.as_bn_bwd_coef_offset():]
    ref = br.bn_bwd64(gad.reshape(-1, 32), zd.reshape(-1, 32), state, gamma)
    sc = br.bwd_scales(gad.reshape(-1, 32), zd.reshape(-1, 32), state, gamma, ref, _bwd_lane(g))
    gz_bound = K_BWD * br.U * sc["g_z"]
    if ref["n_amb"]:
      gz_bound = gz_bound + torch.where(ref["amb"], gamma.double().abs() * state["invstd"].double() *
                                        gad.reshape(-1, 32).double().abs(), torch.zeros_like(gz_bound))
    ratios = {}
    # direct route: stage 3 in the weight-gradient kernel, the next sums in the data gradient
    gz_d = ops.pcl_zeros(g, DEV)
    dW = torch.zeros(32, 32, 3, 3, device=DEV); db = torch.zeros(32, device=DEV)
    wws = torch.empty(lib.as_conv32_wgrad_workspace(g, g, shape), device=DEV)
    nat.call("as_conv32_wgrad_bnapply", nat.ptr(x), g, nat.ptr(gab), nat.ptr(zb), g, shape, nat.ptr(st.scale),
             nat.ptr(st.shift), nat.ptr(st.mean), nat.ptr(coef), 0.2, nat.ptr(gz_d), nat.ptr(dW), nat.ptr(db), 0, nat.ptr(wws),
             nat.stream())
    _check_bwd(tag, ratios, "wgrad_bnapply_g_z", ops.pcl_interior(gz_d, g).reshape(-1, 32), ref["g_z"], gz_bound)
    gx_d, sums_d = ops.conv32_dgrad_bnbwd(gz_d, g, wp_t, shape, gab, znb, stn)
    # minimal-filtering route
    gz_w, gx_w = ops.pcl_zeros(g, DEV), ops.pcl_zeros(g, DEV)
    nws = torch.empty(lib.as_bn_bwd_workspace(g), device=DEV)
    fws = torch.empty(lib.as_conv32_wino_bwd_workspace(), device=DEV)
    nat.call("as_conv32_wino_bwd", nat.ptr(x), g, nat.ptr(gab), nat.ptr(zb), g, shape, nat.ptr(ww_t), nat.ptr(st.scale),
             nat.ptr(st.shift), nat.ptr(st.mean), nat.ptr(coef), 0.2, nat.ptr(znb), nat.ptr(stn.scale), nat.ptr(stn.shift),
             nat.ptr(stn.mean), nat.ptr(gz_w), nat.ptr(gx_w), nat.ptr(dW), nat.ptr(db), 0, nat.ptr(nws), nat.ptr(fws), nat.stream())
    _check_bwd(tag, ratios, "wino_bwd_g_z", ops.pcl_interior(gz_w, g).reshape(-1, 32), ref["g_z"], gz_bound)
    # the next layer's backward from the fused stage-1 sums, against fp64 on the g_x each route stored
    for route, gx, sums, lane in (("fwd_bnbwd", gx_d, sums_d, lane_lds),
                                  ("wino_bwd", gx_w, ops.BnBwdSums(nws, lib.as_conv32_wino_bwd_parts()), lane_wino)):
      gxi = ops.pcl_interior(gx, g).reshape(-1, 32)
      refn = br.bn_bwd64(gxi, znd.reshape(-1, 32), staten, gamman)
      scn = br.bwd_scales(gxi, znd.reshape(-1, 32), staten, gamman, refn, lane)
      g_zn, ggn, gbn = ops.bn_act_bwd(gx, znb, stn, gamman, g, True, sums=sums)
      _check_bwd(tag, ratios, route + "_next_g_gamma", ggn, refn["g_gamma"], K_BWD * br.U * scn["g_gamma"])
      _check_bwd(tag, ratios, route + "_next_g_beta", gbn, refn["g_beta"], K_BWD * br.U * scn["g_beta"])
      bn = K_BWD * br.U * scn["g_z"]
      if refn["n_amb"]:
        bn = bn + torch.where(refn["amb"], gamman.double().abs() * staten["invstd"].double() * gxi.double().abs(),
                              torch.zeros_like(bn))
      _check_bwd(tag, ratios, route + "_next_g_z", ops.pcl_interior(g_zn, g).reshape(-1, 32), refn["g_z"], bn)
    parity_note("bn_bwd[%s]" % tag, n_lane_stage1=_bwd_lane(g), n_lane_fwd_bnbwd=lane_lds, n_lane_wino_bwd=lane_wino,
                ambiguous_branches=ref["n_amb"], **{"worst_err_over_bound_" + k: v for k, v in ratios.items()})
    del zb, gab, znb, gz_d, gz_w, gx_d, gx_w
