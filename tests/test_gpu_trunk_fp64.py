"""The feature trunk's kernels (csrc/trunk.hip) through the C ABI, ONE LAUNCH AT A TIME, against the float64 restatement and the
derived bounds of tests/trunk_ref.py (held to torch on the CPU by tests/test_trunk_ref_cpu.py).  Each launch is judged on the
inputs it actually read: what an earlier launch stored is read back and handed to the reference, so errors do not compound
in a bound.

Every PCL buffer (inputs too) carries one NaN bit pattern in its halo, every output in its interior as well: after a launch
the interior holds no NaN (all of it was written, and no halo word was read into it) and every halo word is bit-unchanged.
dW, db, bn_grads, sums_next, state and the stat partials are slices of larger buffers filled with the same pattern.  No
element is left out of a comparison; every comparison asserts err / bound <= 1 and the worst ratio of every case goes to
conftest.parity_note.

Worst err / bound seen on an MI355X, per quantity (the parity notes trunk[...] of a run hold every case):
  z 0.023, a_out 0.48 (both at 24 x 78 x 6); g_x 0.028; dW 0.77 and db 0.46, both on the 1 x 1 map, where the sum has two terms
  and one rounding is half of the bound (0.02 and below on every larger map); g_z through the centre-tap identity 0.17;
  g_gamma 0.007, g_beta 0.020; sums_next 0.019 (dy) and 0.007 (dx), 0.011 / 0.004 on all-ones gradients; the merged states
  0.50 .. 0.56 (one rounding of an fp64 result against a bound of one ulp); running statistics 0.49.  No ambiguous LeakyReLU
  branch turned up in any case.  The file takes FILE_SECONDS s.
"""
import math
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from adaptive_stereo import _native as nat
from adaptive_stereo import hip_ops as ops
from adaptive_stereo.hip_ops import Pcl
import bn_ref as br
import trunk_ref as tr
from conftest import parity_note
from test_gpu_batchnorm_fp64 import check_producer

DEV = "cuda:0"
PATTERN = 0x7FF92345        # a quiet NaN as a float and (twice) as a double that no arithmetic produces
GUARD = 64
SHAPE = ops.conv_shape_2d(1)


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
  """the file's wall time, into the parity notes"""
  t0 = time.time()
  yield
  parity_note("trunk[wall time of tests/test_gpu_trunk_fp64.py]", seconds=round(time.time() - t0, 1))


# ----------------------------------------------------------------------------- buffers
class PclBuf(object):
  """a PCL buffer full of PATTERN; `fill` ([B, H, W, 32]) goes to the interior"""

  def __init__(self, g, fill=None):
    self.g = g
    self.raw = torch.full((g.numel(),), PATTERN, dtype=torch.int32, device=DEV)
    self.f = self.raw.view(torch.float32)
    if fill is not None:
      ops.pcl_interior(self.f, g)[:, 0].copy_(fill.to(DEV))

  def ptr(self):
    return nat.ptr(self.f)

  def dev_interior(self):
    return ops.pcl_interior(self.f, self.g)[:, 0]

  def halo_untouched(self):
    r = ops.pcl_view(self.raw, self.g).clone()
    g = self.g
    r[:, :, g.ph:g.ph + g.H, g.pw:g.pw + g.W] = PATTERN
    return bool((r == PATTERN).all())

  def all_untouched(self):
    return bool((self.raw == PATTERN).all())

  def interior(self, what):
    torch.cuda.synchronize()
    v = self.dev_interior().cpu()
    assert not bool(torch.isnan(v).any()), "%s: %d interior elements are NaN (not written, or a halo was read)" % (
        what, int(torch.isnan(v).sum()))
    assert self.halo_untouched(), "%s: a halo word was written" % what
    return v


class Guarded(object):
  """numel elements of float32 / float64 inside a buffer filled with PATTERN"""

  def __init__(self, numel, dtype=torch.float32, init=None):
    words = numel * (2 if dtype == torch.float64 else 1)
    self.buf = torch.full((GUARD + words + GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    self.lo, self.hi = GUARD, GUARD + words
    self.view = self.buf[self.lo:self.hi].view(dtype)
    if init is not None:
      self.view.copy_(init.reshape(-1).to(DEV))

  def ptr(self):
    return nat.ptr(self.view)

  def untouched(self):
    return bool((self.buf == PATTERN).all())

  def result(self, what):
    torch.cuda.synchronize()
    b = self.buf.cpu()
    assert bool((b[:self.lo] == PATTERN).all()), "%s: wrote in front of the destination" % what
    assert bool((b[self.hi:] == PATTERN).all()), "%s: wrote behind the destination" % what
    v = self.view.cpu()
    assert not bool(torch.isnan(v).any()), "%s: %d elements not written" % (what, int(torch.isnan(v).sum()))
    return v


def _pcl(geom):
  B, H, W, groups, (ph, pw) = geom
  return Pcl(B, 1, H, W, 0, ph, pw)


def _pack(w, flip):
  return ops.pack_weights(w.to(DEV), SHAPE, flip)


def _identity():
  w = torch.zeros(32, 32, 3, 3)
  w[torch.arange(32), torch.arange(32), 1, 1] = 1.0
  return w


def _tap_perm(kh, kw):
  """one tap times a channel permutation: w[co, perm[co], kh, kw] = 1"""
  perm = torch.randperm(32, generator=torch.Generator().manual_seed(10 + 3 * kh + kw))
  w = torch.zeros(32, 32, 3, 3)
  w[torch.arange(32), perm, kh, kw] = 1.0
  return w, perm


def _shift(t, dy, dx):
  """s[b, y, x] = t[b, y + dy, x + dx], zero outside the map"""
  B, H, W, C = t.shape
  p = torch.nn.functional.pad(t, (0, 0, 1, 1, 1, 1))
  return p[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


class Worst(object):
  def __init__(self, tag):
    self.tag, self.r, self.extra = tag, {}, {}

  def check(self, name, got, ref, bound):
    got, ref = got.double().reshape(ref.shape), ref.double()
    err = (got - ref).abs()
    r = br.worst_ratio(err, bound)
    self.r[name] = max(self.r.get(name, 0.0), r)
    if r > 1.0:
      ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), err * float("inf")).nan_to_num(0.0, posinf=float("inf"))
      i = int(ratio.reshape(-1).argmax())
      idx = tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape)))
      raise AssertionError("%s: %s err/bound %.3g at %s (got %r, reference %r, bound %.3e), %d of %d elements over" % (
          self.tag, name, r, idx, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(bound.reshape(-1)[i]),
          int((ratio > 1).sum()), ratio.numel()))

  def note(self, **extra):
    parity_note("trunk[%s]" % self.tag, **extra, **{"worst_err_over_bound_" + k: v for k, v in self.r.items()})


# ----------------------------------------------------------------------------- launches
class Fwd(object):
  """one as_trunk_fwd launch with guarded outputs"""

  def __init__(self, g, groups, src, w, bias, skip=None, prev=None, gamma=None, beta=None, want_stats=True):
    lib = nat.load()
    self.g, self.groups = g, groups
    self.parts = lib.as_trunk_parts(g, groups)
    assert self.parts >= 1
    self.z = PclBuf(g)
    P = self.parts * groups
    self.keep = [_pack(w, False), bias.to(DEV)]
    if want_stats:
      self.s_mean, self.s_m2, self.s_cnt = Guarded(P * 32), Guarded(P * 32), Guarded(P)
      sp = (self.s_mean.ptr(), self.s_m2.ptr(), self.s_cnt.ptr())
    else:
      sp = (None, None, None)
    if prev is None:
      self.a_out = self.state = None
      nat.call("as_trunk_fwd", src.ptr(), None, None, None, g, groups, nat.ptr(self.keep[0]), nat.ptr(self.keep[1]), br.SLOPE,
               self.z.ptr(), sp[0], sp[1], sp[2], nat.stream())
    else:
      self.a_out = PclBuf(g)
      self.state = Guarded(groups * 160)
      self.keep += [gamma.to(DEV), beta.to(DEV)]
      bn = nat.TrunkBn(prev.s_mean.ptr(), prev.s_m2.ptr(), prev.s_cnt.ptr(), nat.ptr(self.keep[2]), nat.ptr(self.keep[3]),
                       self.state.ptr(), prev.parts, br.EPS)
      nat.call("as_trunk_fwd", src.ptr(), skip.ptr(), bn, self.a_out.ptr(), g, groups, nat.ptr(self.keep[0]),
               nat.ptr(self.keep[1]), br.SLOPE, self.z.ptr(), sp[0], sp[1], sp[2], nat.stream())

  def stats(self, what):
    """(cnt [G*P], mean [G*P, 32], m2) read back, and the same as an ops.StatParts on the device"""
    cnt, mean, m2 = self.s_cnt.result(what + " cnt"), self.s_mean.result(what + " mean"), self.s_m2.result(what + " m2")
    sp = ops.StatParts(self.parts * self.groups, DEV)
    sp.cnt.copy_(self.s_cnt.view); sp.mean.copy_(self.s_mean.view); sp.m2.copy_(self.s_m2.view)
    return cnt, mean.view(-1, 32), m2.view(-1, 32), sp


class Bwd(object):
  """one as_trunk_bwd launch with guarded outputs.  state / state_next: [groups, 5, 32] fp32 (CPU); sums: a device tensor"""

  def __init__(self, g, groups, g_a, x, w, z=None, state=None, sums=None, nparts=0, gamma=None, z_next=None, state_next=None,
               accumulate=0, dW_init=None, db_init=None):
    lib = nat.load()
    self.g, self.groups = g, groups
    self.parts = lib.as_trunk_parts(g, groups)
    self.g_x = PclBuf(g)
    self.dW, self.db = Guarded(9216, init=dW_init), Guarded(32, init=db_init)
    self.ws = torch.empty(lib.as_trunk_bwd_workspace(g, groups), device=DEV)
    self.keep = [_pack(w, True)]
    self.bn_grads = Guarded(groups * 64) if z is not None else None
    if z_next is not None:
      self.sums_next = Guarded(groups * self.parts * 64, torch.float64)
      self.keep.append(state_next.to(DEV).contiguous())
      nx = (z_next.ptr(), nat.ptr(self.keep[-1]), self.sums_next.ptr())
    else:
      self.sums_next, nx = None, (None, None, None)
    if z is None:
      nat.call("as_trunk_bwd", g_a.ptr(), None, None, None, 0, None, None, x.ptr(), nat.ptr(self.keep[0]), self.g_x.ptr(),
               nx[0], nx[1], nx[2], g, groups, br.SLOPE, self.dW.ptr(), self.db.ptr(), accumulate, nat.ptr(self.ws), nat.stream())
    else:
      self.keep += [state.to(DEV).contiguous(), gamma.to(DEV)]
      nat.call("as_trunk_bwd", g_a.ptr(), z.ptr(), nat.ptr(self.keep[-2]), nat.ptr(sums), nparts, nat.ptr(self.keep[-1]),
               self.bn_grads.ptr(), x.ptr(), nat.ptr(self.keep[0]), self.g_x.ptr(), nx[0], nx[1], nx[2], g, groups, br.SLOPE,
               self.dW.ptr(), self.db.ptr(), accumulate, nat.ptr(self.ws), nat.stream())

  def sums(self, what):
    """the per-workgroup partials summed per group in fp64: (sum_dy, sum_dx) [groups, 32]"""
    s = self.sums_next.result(what + " sums_next").view(self.groups, self.parts, 64).sum(1)
    return s[:, :32], s[:, 32:]


def _check_sums(wst, bwd, gx_stored, z_next, state_next, groups, n_lane, what, max_amb=0):
  ref = tr.next_sums(gx_stored, z_next, state_next, groups, n_lane)
  assert ref["n_amb"] <= max_amb, "%s: %d ambiguous branches in the layer below" % (what, ref["n_amb"])
  sdy, sdx = bwd.sums(what)
  wst.check("sums_next_dy", sdy, ref["sum_dy"], ref["e_sum_dy"])
  wst.check("sums_next_dx", sdx, ref["sum_dx"], ref["e_sum_dx"])
  return ref["n_amb"]


# ============================================================================= single taps, exact
TAP_GEOMS = [tr.GEOMS[1], tr.GEOMS[4], tr.GEOMS[5], tr.GEOMS[8]]


@pytest.mark.parametrize("geom", TAP_GEOMS, ids=tr.geom_id)
def test_single_tap_is_a_shift_bit_for_bit(geom):
  """Weights of one tap (kh, kw) times a channel permutation, bias 0, each of the nine taps.  Forward MODE 0: z is the shifted,
  permuted input bit for bit, zeros where the tap leaves the map.  Backward MODE 0: g_x is the mirrored shift through the
  inverse permutation.  Pins tap order, mirroring, the transpose_flip packing and the channel order with no tolerance."""
  B, H, W, groups, _ = geom
  g = _pcl(geom)
  gen = torch.Generator().manual_seed(tr.case_seed(geom, 31))
  a = torch.randn(B, H, W, 32, generator=gen) * tr.chan_scale()
  ga = torch.randn(B, H, W, 32, generator=gen)
  ab, gab = PclBuf(g, a), PclBuf(g, ga)
  for kh in range(3):
    for kw in range(3):
      w, perm = _tap_perm(kh, kw)
      tag = "%s tap (%d, %d)" % (tr.geom_id(geom), kh, kw)
      f = Fwd(g, groups, ab, w, torch.zeros(32), want_stats=False)
      z = f.z.interior(tag + " z")
      assert torch.equal(z, _shift(a, kh - 1, kw - 1)[..., perm]), tag + ": forward is not the shifted, permuted input"
      b = Bwd(g, groups, gab, ab, w)
      gx = b.g_x.interior(tag + " g_x")
      inv = torch.argsort(perm)
      assert torch.equal(gx, _shift(ga, 1 - kh, 1 - kw)[..., inv]), tag + ": backward is not the mirrored shift"
      b.dW.result(tag + " dW"); b.db.result(tag + " db")


@pytest.mark.parametrize("geom", [tr.GEOMS[4], tr.GEOMS[6]], ids=tr.geom_id)
def test_weight_gradient_of_two_impulses_is_one_tap(geom):
  """x one voxel and channel, g_a one voxel and channel, a tap apart: dW is their product at [co, ci, kh, kw] and exactly zero
  elsewhere, db is the impulse, for each of the nine taps, the g_a impulse inside the shifted last tile's overlap and at the
  seam (a `dup` lane counted twice would double it)."""
  B, H, W, groups, _ = geom
  g = _pcl(geom)
  seam = tr.tiling(B, H, W, groups)["seam"]
  y_g = 1
  for n, (kh, kw) in enumerate([(a, b) for a in range(3) for b in range(3)]):
    x0 = (seam + 2, seam, W - 2)[n % 3]              # inside the overlap / first column of the shifted tile / next to the end
    b_img = n % B
    yx, xx = y_g + kh - 1, x0 + kw - 1
    co, ci = (5 + 3 * n) % 32, (11 + 7 * n) % 32
    x = torch.zeros(B, H, W, 32); ga = torch.zeros(B, H, W, 32)
    x[b_img, yx, xx, ci] = 1.5
    ga[b_img, y_g, x0, co] = -2.25
    bw = Bwd(g, groups, PclBuf(g, ga), PclBuf(g, x), _identity())
    tag = "%s impulse tap (%d, %d)" % (tr.geom_id(geom), kh, kw)
    dW = bw.dW.result(tag + " dW").view(32, 32, 3, 3)
    exp = torch.zeros(32, 32, 3, 3); exp[co, ci, kh, kw] = 1.5 * -2.25
    assert torch.equal(dW, exp), "%s: dW has %d wrong entries, [co, ci, kh, kw] = %s holds %r" % (
        tag, int((dW != exp).sum()), (co, ci, kh, kw), float(dW[co, ci, kh, kw]))
    edb = torch.zeros(32); edb[co] = -2.25
    assert torch.equal(bw.db.result(tag + " db"), edb), tag + ": db"
    assert torch.equal(bw.g_x.interior(tag + " g_x"), ga), tag + ": g_x of the identity"


# ============================================================================= forward MODE 1
def _merge_check(wst, tag, cnt, mean, m2, P, groups, gamma, beta, state):
  """both groups' published states against the fp64 merge of the partials the launch read (bn_ref.merge_bounds)"""
  for gi in range(groups):
    c, mu, q = cnt[gi * P:(gi + 1) * P], mean[gi * P:(gi + 1) * P], m2[gi * P:(gi + 1) * P]
    n, mu64, q64 = br.chan_merge64(c, mu, q)
    ref = br.bn_state64(n, mu64, q64, gamma, beta, torch.zeros(32), torch.ones(32))
    bnd = br.merge_bounds(c, mu, q, gamma, ref, c=P + 32)
    for f in ("mean", "invstd", "scale", "shift", "var_u"):
      wst.check("state_" + f, state[f][gi], ref[f], bnd[f])


def _forward_mode1(geom, fam, wst):
  B, H, W, groups, _ = geom
  g = _pcl(geom)
  c = tr.fwd_case(fam, geom)
  tag = wst.tag
  f0 = Fwd(g, groups, PclBuf(g, c["src"]), _identity(), torch.zeros(32))
  z0 = f0.z.interior(tag + " z of the identity")
  assert torch.equal(z0, c["src"]), tag + ": the centre-tap identity must copy its input"
  cnt, mean, m2, _ = f0.stats(tag + " partials of launch 0")
  skip = PclBuf(g, c["skip"])
  f1 = Fwd(g, groups, f0.z, c["w"], c["bias"], skip=skip, prev=f0, gamma=c["gamma"], beta=c["beta"])
  a_out, z = f1.a_out.interior(tag + " a_out"), f1.z.interior(tag + " z")
  state = tr.state_from_kernel(f1.state.result(tag + " state").view(groups, 5, 32))
  _merge_check(wst, tag, cnt, mean, m2, f0.parts, groups, c["gamma"], c["beta"], state)
  if groups == 2:
    assert not torch.equal(state["mean"][0], state["mean"][1])
  ref = tr.forward_layer(z0, c["w"], c["bias"], skip=c["skip"], state=state, groups=groups)
  assert ref["n_amb"] <= 2, "%s: %d ambiguous branches" % (tag, ref["n_amb"])
  wst.check("a_out", a_out, ref["a"], ref["e_a"])
  wst.check("z", z, ref["z"], ref["e_z"])
  if fam == "shift_large":       # teeth: a halo of lrelu(shift) instead of zero moves a border voxel by 100 * sum w ~ 50
    assert float(ref["e_z"].max()) < 1.0
  _, _, _, sp = f1.stats(tag + " partials of launch 1")
  merges = math.ceil(B * H * W / groups / f1.parts / 32) + 8
  check_producer("trunk MODE 1 " + tag, f1.z.dev_interior().contiguous(), sp, merges, groups=groups)
  assert f0.z.halo_untouched() and skip.halo_untouched()
  return ref["n_amb"]


@pytest.mark.parametrize("geom", tr.GEOMS, ids=tr.geom_id)
def test_forward_mode1_against_fp64(geom):
  """as_trunk_fwd with a BatchNorm in front: the partials come from a real MODE 0 launch (the centre-tap identity on a crafted
  src, bit-exact), both groups' published states against the fp64 merge, a_out element-wise against lrelu(src * scale + shift)
  + skip from the PUBLISHED state, z against the fp64 convolution of that operand with zero padding, the moments left for the
  next layer through check_producer's model.  Families: trunk_ref.fwd_case."""
  wst = Worst(tr.geom_id(geom))
  n_amb = 0
  for fam in tr.FWD_FAMILIES:
    wst.tag = "%s %s" % (tr.geom_id(geom), fam)
    n_amb += _forward_mode1(geom, fam, wst)
  wst.tag = "fwd1 " + tr.geom_id(geom)
  wst.note(ambiguous_branches=n_amb)


# ============================================================================= backward
def _ones_state(groups, shift):
  st = torch.zeros(groups, 5, 32)
  st[:, 1] = 1.0; st[:, 2] = 1.0; st[:, 3] = shift; st[:, 4] = 1.0
  return st


@pytest.mark.parametrize("geom", tr.GEOMS, ids=tr.geom_id)
def test_backward_mode0_against_fp64(geom):
  """as_trunk_bwd as conv_alone: g_x, dW, db against fp64 and sums_next, read back per workgroup partial in fp64, against the
  sums over each group's voxels ONCE.  Then an all-ones gradient through the identity with a state of the layer below that is
  positive (negative) everywhere: every term is 1 (slope), so a `dup` lane counted twice or a valid one dropped is off by a
  whole term; sums_next[0] must be the voxel count (times slope)."""
  B, H, W, groups, _ = geom
  g = _pcl(geom)
  t = tr.tiling(B, H, W, groups)
  wst = Worst("bwd0 " + tr.geom_id(geom))
  c = tr.bwd_case("zero_mean", geom)
  w, _ = tr.random_weights(tr.case_seed(geom, 41))
  stn, stn_t = tr.craft_state(c["z_next"], c["gamma_next"], groups, c["beta_next"])
  gab, xb, znb = PclBuf(g, c["g_a"]), PclBuf(g, c["x"]), PclBuf(g, c["z_next"])
  b = Bwd(g, groups, gab, xb, w, z_next=znb, state_next=stn_t)
  assert b.parts == t["gper"]
  ref = tr.backward_layer(c["g_a"], c["x"], w)
  gx = b.g_x.interior(wst.tag + " g_x")
  wst.check("g_x", gx, ref["g_x"], ref["e_g_x"])
  wst.check("dW", b.dW.result(wst.tag + " dW").view(32, 32, 3, 3), ref["dW"], ref["e_dW"])
  wst.check("db", b.db.result(wst.tag + " db"), ref["db"], ref["e_db"])
  _check_sums(wst, b, gx, c["z_next"], stn, groups, t["n_lane"], wst.tag)
  per_group = B // groups * H * W
  ones = PclBuf(g, torch.ones(B, H, W, 32))
  for shift, factor in ((1000.0, 1.0), (-1000.0, br.SLOPE)):
    st_t = _ones_state(groups, shift)
    st = tr.state_from_kernel(st_t)
    b1 = Bwd(g, groups, ones, xb, _identity(), z_next=znb, state_next=st_t)
    gx1 = b1.g_x.interior(wst.tag + " g_x of ones")
    assert torch.equal(gx1, torch.ones(B, H, W, 32))
    refn = tr.next_sums(gx1, c["z_next"], st, groups, t["n_lane"])
    sdy, sdx = b1.sums(wst.tag + " ones")
    assert bool(((refn["sum_dy"] - factor * per_group).abs() <= 1e-9 * per_group).all())
    assert bool((refn["e_sum_dy"] < 0.25 * factor).all()), "the bound cannot see one term"
    wst.check("sums_next_dy_ones", sdy, refn["sum_dy"], refn["e_sum_dy"])
    wst.check("sums_next_dx_ones", sdx, refn["sum_dx"], refn["e_sum_dx"])
    if factor == 1.0:
      assert bool((sdy == float(per_group)).all()), "a sum of ones is exact: %r != %d" % (float(sdy[0, 0]), per_group)
    # db of the identity: the count of the whole launch, exactly
    assert bool((b1.db.result(wst.tag + " db of ones") == float(B * H * W)).all())
  assert gab.halo_untouched() and xb.halo_untouched() and znb.halo_untouched()
  wst.note(gper=b.parts, n_lane=t["n_lane"])


def _sums_by_mode0(g, groups, g_a, z_buf, state_t, xb):
  """this layer's stage-1 partial sums the way production gets them: from the launch above.  A MODE 0 launch of the centre-tap
  identity stores g_x = g_a bit for bit and leaves the sums of (g_a, z, state); returns (the g_x buffer, the launch)"""
  b = Bwd(g, groups, PclBuf(g, g_a), xb, _identity(), z_next=z_buf, state_next=state_t)
  return b.g_x, b


@pytest.mark.parametrize("geom", tr.GEOMS, ids=tr.geom_id)
def test_backward_mode1_against_fp64(geom):
  """as_trunk_bwd on a BasicBlock, states crafted from fp64 moments, `sums` from a preceding MODE 0 launch (nparts is the real
  gper): g_x with the skip term, dW and db over both groups, bn_grads per group, sums_next for the layer below; every family of
  trunk_ref.bwd_case; accumulate 0 and 1 (1: dW, db start from a known tensor and end at the fp32 sum of that and the
  accumulate-0 result, bit for bit)."""
  B, H, W, groups, _ = geom
  g = _pcl(geom)
  t = tr.tiling(B, H, W, groups)
  wst = Worst(tr.geom_id(geom))
  w, _ = tr.random_weights(tr.case_seed(geom, 51))
  for fam in tr.BWD_FAMILIES:
    wst.tag = tag = "bwd1 %s %s" % (tr.geom_id(geom), fam)
    c = tr.bwd_case(fam, geom)
    st, st_t = tr.craft_state(c["z"], c["gamma"], groups, c["beta"])
    stn, stn_t = tr.craft_state(c["z_next"], c["gamma_next"], groups, c["beta_next"])
    xb, zb, znb = PclBuf(g, c["x"]), PclBuf(g, c["z"]), PclBuf(g, c["z_next"])
    gab, above = _sums_by_mode0(g, groups, c["g_a"], zb, st_t, xb)
    assert torch.equal(gab.interior(tag + " g_x of the launch above"), c["g_a"])
    _check_sums(wst, above, c["g_a"], c["z"], st, groups, t["n_lane"], tag + " (launch above)")
    b = Bwd(g, groups, gab, xb, w, z=zb, state=st_t, sums=above.sums_next.view, nparts=above.parts, gamma=c["gamma"],
            z_next=znb, state_next=stn_t)
    ref = tr.backward_layer(c["g_a"], c["x"], w, z=c["z"], state=st, gamma=c["gamma"], groups=groups, n_lane=t["n_lane"])
    assert ref["n_amb"] == 0, "%s: %d ambiguous branches with a crafted state" % (tag, ref["n_amb"])
    gx = b.g_x.interior(tag + " g_x")
    dW, db = b.dW.result(tag + " dW"), b.db.result(tag + " db")
    wst.check("g_x", gx, ref["g_x"], ref["e_g_x"])
    wst.check("dW", dW.view(32, 32, 3, 3), ref["dW"], ref["e_dW"])
    wst.check("db", db, ref["db"], ref["e_db"])
    bg = b.bn_grads.result(tag + " bn_grads").view(groups, 2, 32)
    wst.check("g_gamma", bg[:, 0], ref["g_gamma"], ref["e_g_gamma"])
    wst.check("g_beta", bg[:, 1], ref["g_beta"], ref["e_g_beta"])
    _check_sums(wst, b, gx, c["z_next"], stn, groups, t["n_lane"], tag)
    if fam == "sent_edges":      # teeth: a sentinel dropped from (or counted twice in) db or g_beta shows far above the bounds
      assert bool((ref["e_g_beta"] < 0.1 * 1e4 * br.SLOPE).all())
    # accumulate = 1 on top of a known tensor
    gen = torch.Generator().manual_seed(5)
    dW0, db0 = torch.randn(9216, generator=gen), torch.randn(32, generator=gen)
    b2 = Bwd(g, groups, gab, xb, w, z=zb, state=st_t, sums=above.sums_next.view, nparts=above.parts, gamma=c["gamma"],
             z_next=znb, state_next=stn_t, accumulate=1, dW_init=dW0, db_init=db0)
    assert torch.equal(b2.dW.result(tag + " dW accumulated"), dW0 + dW), tag + ": accumulate = 1 is not init + dW in fp32"
    assert torch.equal(b2.db.result(tag + " db accumulated"), db0 + db), tag + ": accumulate = 1 is not init + db in fp32"
    assert torch.equal(b2.g_x.interior(tag + " g_x again"), gx)
    for buf in (xb, zb, znb, gab):
      assert buf.halo_untouched(), tag + ": an input's halo changed"
  wst.tag = "bwd1 " + tr.geom_id(geom)
  wst.note(gper=t["gper"], n_lane=t["n_lane"], ambiguous_branches=0)


@pytest.mark.parametrize("geom", [tr.GEOMS[1], tr.GEOMS[5], tr.GEOMS[9]], ids=tr.geom_id)
def test_centre_tap_identity_exposes_g_z(geom):
  """MODE 1 with the centre-tap identity: g_x = fl(g_z + g_a), so g_x - g_a is g_z itself: against bn_bwd64 at the bound of the
  stage-3 tests (trunk_ref's e_gz) plus one rounding of the add"""
  B, H, W, groups, _ = geom
  g = _pcl(geom)
  t = tr.tiling(B, H, W, groups)
  wst = Worst("g_z " + tr.geom_id(geom))
  for fam in ("zero_mean", "common_mode", "z_offset"):
    c = tr.bwd_case(fam, geom)
    st, st_t = tr.craft_state(c["z"], c["gamma"], groups, c["beta"])
    xb, zb = PclBuf(g, c["x"]), PclBuf(g, c["z"])
    gab, above = _sums_by_mode0(g, groups, c["g_a"], zb, st_t, xb)
    b = Bwd(g, groups, gab, xb, _identity(), z=zb, state=st_t, sums=above.sums_next.view, nparts=above.parts, gamma=c["gamma"])
    ref = tr.backward_layer(c["g_a"], c["x"], _identity(), z=c["z"], state=st, gamma=c["gamma"], groups=groups, n_lane=t["n_lane"])
    assert ref["n_amb"] == 0
    gx = b.g_x.interior(wst.tag + " g_x").double()
    wst.check("g_z_" + fam, gx - c["g_a"].double(), ref["g_z"], ref["e_gz"] + br.U * (ref["g_z"] + c["g_a"].double()).abs() * 1.0000001)
  wst.note(n_lane=t["n_lane"])


# ============================================================================= the hand-over between launches
@pytest.mark.parametrize("geom", [tr.GEOMS[5], tr.GEOMS[10]], ids=tr.geom_id)
def test_hand_over_forward_and_backward_launch_by_launch(geom):
  """Forward layers 0, 1, 2 (two BasicBlocks and conv_alone's operand), then backward 2, 1, 0, through the C ABI as
  hip_ops.FeatureExtractorFn wires them; every launch judged against fp64 OF THE BUFFERS THE PREVIOUS LAUNCH STORED: the
  buffers, states and sums one launch leaves are what the next one reads.  The states come from the kernel's merge here, so a
  case may widen the bound on at most 2 ambiguous elements (counted and reported)."""
  B, H, W, groups, _ = geom
  g = _pcl(geom)
  t = tr.tiling(B, H, W, groups)
  wst = Worst("chain " + tr.geom_id(geom))
  gen = torch.Generator().manual_seed(tr.case_seed(geom, 61))
  a0 = torch.randn(B, H, W, 32, generator=gen)
  a0[B // groups:] += 0.5
  g_out = torch.randn(B, H, W, 32, generator=gen)
  ws = [tr.random_weights(tr.case_seed(geom, 62 + l)) for l in range(3)]
  gam = [torch.rand(32, generator=gen) + 0.5 for _ in range(2)]
  bet = [torch.randn(32, generator=gen) * 0.5 for _ in range(2)]
  n_amb = 0
  # forward
  a0b = PclBuf(g, a0)
  f0 = Fwd(g, groups, a0b, ws[0][0], ws[0][1])
  z0 = f0.z.interior("chain z0")
  r = tr.forward_layer(a0, ws[0][0], ws[0][1])
  wst.check("z_layer0", z0, r["z"], r["e_z"])
  f1 = Fwd(g, groups, f0.z, ws[1][0], ws[1][1], skip=a0b, prev=f0, gamma=gam[0], beta=bet[0])
  a1, z1 = f1.a_out.interior("chain a1"), f1.z.interior("chain z1")
  st0_t = f1.state.result("chain state 0").view(groups, 5, 32)
  st0 = tr.state_from_kernel(st0_t)
  cnt, mean, m2, _ = f0.stats("chain partials 0")
  _merge_check(wst, "chain", cnt, mean, m2, f0.parts, groups, gam[0], bet[0], st0)
  r = tr.forward_layer(z0, ws[1][0], ws[1][1], skip=a0, state=st0, groups=groups)
  n_amb += r["n_amb"]
  wst.check("a_out_layer1", a1, r["a"], r["e_a"]); wst.check("z_layer1", z1, r["z"], r["e_z"])
  f2 = Fwd(g, groups, f1.z, ws[2][0], ws[2][1], skip=f1.a_out, prev=f1, gamma=gam[1], beta=bet[1], want_stats=False)
  a2, out = f2.a_out.interior("chain a2"), f2.z.interior("chain out")
  st1_t = f2.state.result("chain state 1").view(groups, 5, 32)
  st1 = tr.state_from_kernel(st1_t)
  cnt, mean, m2, _ = f1.stats("chain partials 1")
  _merge_check(wst, "chain", cnt, mean, m2, f1.parts, groups, gam[1], bet[1], st1)
  r = tr.forward_layer(z1, ws[2][0], ws[2][1], skip=a1, state=st1, groups=groups)
  n_amb += r["n_amb"]
  wst.check("a_out_layer2", a2, r["a"], r["e_a"]); wst.check("z_layer2", out, r["z"], r["e_z"])
  # backward: conv_alone, then the two blocks
  gob = PclBuf(g, g_out)
  b2 = Bwd(g, groups, gob, f2.a_out, ws[2][0], z_next=f1.z, state_next=st1_t)
  r = tr.backward_layer(g_out, a2, ws[2][0])
  gx2 = b2.g_x.interior("chain g_x2")
  wst.check("g_x_layer2", gx2, r["g_x"], r["e_g_x"])
  wst.check("dW_layer2", b2.dW.result("chain dW2").view(32, 32, 3, 3), r["dW"], r["e_dW"])
  wst.check("db_layer2", b2.db.result("chain db2"), r["db"], r["e_db"])
  n_amb += _check_sums(wst, b2, gx2, z1, st1, groups, t["n_lane"], "chain launch 2", max_amb=2)
  b1 = Bwd(g, groups, b2.g_x, f1.a_out, ws[1][0], z=f1.z, state=st1_t, sums=b2.sums_next.view, nparts=b2.parts, gamma=gam[1],
           z_next=f0.z, state_next=st0_t)
  r = tr.backward_layer(gx2, a1, ws[1][0], z=z1, state=st1, gamma=gam[1], groups=groups, n_lane=t["n_lane"])
  gx1 = b1.g_x.interior("chain g_x1")
  bg = b1.bn_grads.result("chain bn_grads 1").view(groups, 2, 32)
  for name, got in (("g_x", gx1), ("dW", b1.dW.result("chain dW1").view(32, 32, 3, 3)), ("db", b1.db.result("chain db1")),
                    ("g_gamma", bg[:, 0]), ("g_beta", bg[:, 1])):
    wst.check(name + "_layer1", got, r[name], r["e_" + name])
  n_amb += _check_sums(wst, b1, gx1, z0, st0, groups, t["n_lane"], "chain launch 1", max_amb=2)
  b0 = Bwd(g, groups, b1.g_x, a0b, ws[0][0], z=f0.z, state=st0_t, sums=b1.sums_next.view, nparts=b1.parts, gamma=gam[0])
  r = tr.backward_layer(gx1, a0, ws[0][0], z=z0, state=st0, gamma=gam[0], groups=groups, n_lane=t["n_lane"])
  bg = b0.bn_grads.result("chain bn_grads 0").view(groups, 2, 32)
  for name, got in (("g_x", b0.g_x.interior("chain g_x0")), ("dW", b0.dW.result("chain dW0").view(32, 32, 3, 3)),
                    ("db", b0.db.result("chain db0")), ("g_gamma", bg[:, 0]), ("g_beta", bg[:, 1])):
    wst.check(name + "_layer0", got, r[name], r["e_" + name])
  assert n_amb <= 2, "chain: %d ambiguous branches" % n_amb
  for buf in (a0b, f0.z, f1.z, f1.a_out, f2.a_out, gob, b2.g_x, b1.g_x):
    assert buf.halo_untouched()
  wst.note(ambiguous_branches=n_amb, gper=t["gper"])


# ============================================================================= the small kernels
@pytest.mark.parametrize("B,H,W,halo", [(2, 9, 44, (1, 3)), (4, 3, 33, (2, 2)), (6, 5, 78, (1, 1))])
def test_begin_bwd_is_a_bit_exact_transpose(B, H, W, halo):
  """as_trunk_begin_bwd: NCHW -> PCL bit for bit, the halo untouched, W no multiple of 32; two tensors (nA = B / 2) and one
  (nA = B, g_b null)"""
  g = Pcl(B, 1, H, W, 0, *halo)
  t = torch.randn(B, 32, H, W, generator=torch.Generator().manual_seed(B + W))
  td = t.to(DEV)
  for nA in (B // 2, B):
    out = PclBuf(g)
    ga = td[:nA].contiguous()
    gb = td[nA:].contiguous() if nA < B else None
    nat.call("as_trunk_begin_bwd", nat.ptr(ga), nat.ptr(gb), nA, g, out.ptr(), nat.stream())
    assert torch.equal(out.interior("begin_bwd nA %d" % nA), t.permute(0, 2, 3, 1))


@pytest.mark.parametrize("nlayers", [0, 1, 6])
def test_finish_fwd_transpose_and_running_statistics(nlayers):
  """as_trunk_finish_fwd: PCL -> NCHW bit for bit; the running statistics from a crafted `states` after the two sequential
  group updates, group 0 FIRST (the groups' means are 100 apart, so the order shows), within one fp32 ulp per update of the
  unrounded fp64 result"""
  B, H, W, groups = 2, 5, 44, 2
  g = Pcl(B, 1, H, W, 0, 1, 3)
  gen = torch.Generator().manual_seed(70 + nlayers)
  feats = torch.randn(B, H, W, 32, generator=gen)
  fb = PclBuf(g, feats)
  out = Guarded(B * 32 * H * W)
  nl = max(nlayers, 1)
  states = torch.randn(nl, groups, 5, 32, generator=gen)
  states[:, 1, 0] += 100.0
  states[:, :, 4] = states[:, :, 4].abs() + 0.1
  rm0, rv0 = torch.randn(nl, 32, generator=gen), torch.rand(nl, 32, generator=gen) + 0.5
  rms = [Guarded(32, init=rm0[l]) for l in range(nlayers)]
  rvs = [Guarded(32, init=rv0[l]) for l in range(nlayers)]
  sd = states.to(DEV)
  nat.call("as_trunk_finish_fwd", fb.ptr(), g, out.ptr(), nat.ptr(sd) if nlayers else None, nlayers, groups,
           ops._host_ptrs([r.view for r in rms]) if nlayers else None, ops._host_ptrs([r.view for r in rvs]) if nlayers else None,
           br.MOMENTUM, nat.stream())
  assert torch.equal(out.result("finish_fwd feats").view(B, 32, H, W), feats.permute(0, 3, 1, 2))
  assert fb.halo_untouched()
  wst = Worst("finish_fwd nlayers %d" % nlayers)
  for l in range(nlayers):
    m, v, e_m, e_v = tr.running_update(states[l], rm0[l], rv0[l], br.MOMENTUM)
    wst.check("running_mean", rms[l].result("running_mean %d" % l), m, e_m)
    wst.check("running_var", rvs[l].result("running_var %d" % l), v, e_v)
    swapped, _, _, _ = tr.running_update(states[l].flip(0), rm0[l], rv0[l], br.MOMENTUM)
    assert bool(((swapped - m).abs() > 100 * e_m).all())
  wst.note()


@pytest.mark.parametrize("accumulate", [0, 1])
def test_finish_bwd_adds_the_groups_in_call_order(accumulate):
  """as_trunk_finish_bwd: ((dst or 0) + g0) + g1 in fp32, in that order, bit for bit"""
  nl, groups = 6, 2
  gen = torch.Generator().manual_seed(80)
  bn = torch.randn(nl, groups, 2, 32, generator=gen) * torch.tensor([1.0, 1e3]).view(1, 2, 1, 1)
  init = torch.randn(nl, 2, 32, generator=gen) * 30
  gg = [Guarded(32, init=init[l, 0]) for l in range(nl)]
  gb = [Guarded(32, init=init[l, 1]) for l in range(nl)]
  bd = bn.to(DEV)
  nat.call("as_trunk_finish_bwd", nat.ptr(bd), nl, groups, ops._host_ptrs([t.view for t in gg]), ops._host_ptrs([t.view for t in gb]),
           accumulate, nat.stream())
  for l in range(nl):
    for which, dst in ((0, gg[l]), (1, gb[l])):
      base = init[l, which] if accumulate else torch.zeros(32)
      assert torch.equal(dst.result("finish_bwd"), (base + bn[l, 0, which]) + bn[l, 1, which])


# ============================================================================= refusals and determinism
def test_refusals_leave_the_destination_alone():
  """every unsupported call returns an error and writes nothing: three groups, a batch that does not split into the groups
  (three images, two groups), D != 1, pd != 0, ph = 0, aliased buffers, stat pointers given in part, z_next without
  state_next, a MODE 1 call with an incomplete as_trunk_bn"""
  lib = nat.load()
  good = Pcl(2, 1, 6, 16, 0, 1, 1)
  three = Pcl(3, 1, 6, 16, 0, 1, 1)
  assert lib.as_trunk_parts(three, 1) == 18 and lib.as_trunk_parts(three, 2) == -1 and lib.as_trunk_parts(three, 3) == -1
  assert lib.as_trunk_bwd_workspace(three, 2) == -1
  wp = _pack(_identity(), False)
  bias = torch.zeros(32, device=DEV)
  st = nat.stream()

  def fwd(g, groups, src=None, z=None, stats=(None, None, None), skip=None, bn=None, a_out=None):
    z = z if z is not None else PclBuf(g)
    src = src if src is not None else PclBuf(g, torch.zeros(g.B, g.H, g.W, 32)) if g.D == 1 and g.pd == 0 else PclBuf(g)
    rc = lib.as_trunk_fwd(src.ptr(), skip.ptr() if skip else None, bn, a_out.ptr() if a_out else None, g, groups, nat.ptr(wp),
                          nat.ptr(bias), br.SLOPE, z.ptr(), stats[0], stats[1], stats[2], st)
    torch.cuda.synchronize()
    return rc, z

  for what, g, groups in (("three groups", three, 3), ("3 images in 2 groups", three, 2), ("D = 2", Pcl(2, 2, 6, 16, 0, 1, 1), 2),
                          ("pd = 1", Pcl(2, 1, 6, 16, 1, 1, 1), 2), ("ph = 0", Pcl(2, 1, 6, 16, 0, 0, 1), 2)):
    rc, z = fwd(g, groups)
    assert rc != 0 and z.all_untouched(), "as_trunk_fwd accepted %s" % what
    gx, dW, db = PclBuf(g), Guarded(9216), Guarded(32)
    ws = torch.empty(2 * 18 * (9 * 1024 + 32), device=DEV)
    a, x = PclBuf(g), PclBuf(g)
    rc = lib.as_trunk_bwd(a.ptr(), None, None, None, 0, None, None, x.ptr(), nat.ptr(wp), gx.ptr(), None, None, None, g, groups,
                          br.SLOPE, dW.ptr(), db.ptr(), 0, nat.ptr(ws), st)
    torch.cuda.synchronize()
    assert rc != 0 and gx.all_untouched() and dW.untouched() and db.untouched(), "as_trunk_bwd accepted %s" % what
  # aliases and incomplete argument sets on a good geometry
  src = PclBuf(good, torch.zeros(2, 6, 16, 32))
  before = src.raw.clone()
  rc, _ = fwd(good, 2, src=src, z=src)
  assert rc != 0 and torch.equal(src.raw, before), "z aliasing src"
  sm, s2, sc = Guarded(2 * 18 * 32), Guarded(2 * 18 * 32), Guarded(2 * 18)
  for stats in ((sm.ptr(), None, None), (sm.ptr(), s2.ptr(), None), (None, s2.ptr(), sc.ptr())):
    rc, z = fwd(good, 2, src=src, stats=stats)
    assert rc != 0 and z.all_untouched() and sm.untouched() and s2.untouched() and sc.untouched(), "stat pointers in part"
  gam = torch.ones(32, device=DEV)
  state = Guarded(320)
  skip, a_out = PclBuf(good, torch.zeros(2, 6, 16, 32)), PclBuf(good)
  full = dict(stat_mean=sm.ptr(), stat_m2=s2.ptr(), stat_cnt=sc.ptr(), gamma=nat.ptr(gam), beta=nat.ptr(gam), state=state.ptr())
  for missing in ("stat_mean", "stat_m2", "stat_cnt", "gamma", "beta", "state", "nparts", "skip", "a_out"):
    args = dict(full)
    if missing in args:
      args[missing] = None
    bn = nat.TrunkBn(args["stat_mean"], args["stat_m2"], args["stat_cnt"], args["gamma"], args["beta"], args["state"],
                     0 if missing == "nparts" else 18, br.EPS)
    rc, z = fwd(good, 2, src=src, skip=None if missing == "skip" else skip, bn=bn, a_out=None if missing == "a_out" else a_out)
    assert rc != 0 and z.all_untouched() and a_out.all_untouched() and state.untouched(), "MODE 1 without %s" % missing
  # backward
  ws = torch.empty(lib.as_trunk_bwd_workspace(good, 2), device=DEV)
  ga, x, z = (PclBuf(good, torch.zeros(2, 6, 16, 32)) for _ in range(3))
  stt = torch.ones(2, 5, 32, device=DEV)
  sums = torch.zeros(2 * 18 * 64, dtype=torch.float64, device=DEV)
  bng = Guarded(128)
  dW, db = Guarded(9216), Guarded(32)
  for what, gx in (("g_a", ga), ("x", x), ("z", z)):
    before = gx.raw.clone()
    rc = lib.as_trunk_bwd(ga.ptr(), z.ptr(), nat.ptr(stt), nat.ptr(sums), 18, nat.ptr(gam), bng.ptr(), x.ptr(), nat.ptr(wp), gx.ptr(),
                          None, None, None, good, 2, br.SLOPE, dW.ptr(), db.ptr(), 0, nat.ptr(ws), st)
    torch.cuda.synchronize()
    assert rc != 0 and torch.equal(gx.raw, before) and dW.untouched() and db.untouched() and bng.untouched(), "g_x aliasing " + what
  gx = PclBuf(good)
  sn = Guarded(2 * 18 * 64, torch.float64)
  for what, nx in (("z_next without state_next", (z.ptr(), None, sn.ptr())), ("z_next alone", (z.ptr(), None, None)),
                   ("state_next alone", (None, nat.ptr(stt), None))):
    rc = lib.as_trunk_bwd(ga.ptr(), None, None, None, 0, None, None, x.ptr(), nat.ptr(wp), gx.ptr(), nx[0], nx[1], nx[2], good, 2,
                          br.SLOPE, dW.ptr(), db.ptr(), 0, nat.ptr(ws), st)
    torch.cuda.synchronize()
    assert rc != 0 and gx.all_untouched() and dW.untouched() and db.untouched() and sn.untouched(), what
  for what, margs in (("state", (None, nat.ptr(sums), 18, nat.ptr(gam), bng.ptr())), ("sums", (nat.ptr(stt), None, 18, nat.ptr(gam), bng.ptr())),
                      ("nparts", (nat.ptr(stt), nat.ptr(sums), 0, nat.ptr(gam), bng.ptr())),
                      ("gamma", (nat.ptr(stt), nat.ptr(sums), 18, None, bng.ptr())), ("bn_grads", (nat.ptr(stt), nat.ptr(sums), 18, nat.ptr(gam), None))):
    rc = lib.as_trunk_bwd(ga.ptr(), z.ptr(), margs[0], margs[1], margs[2], margs[3], margs[4], x.ptr(), nat.ptr(wp), gx.ptr(),
                          None, None, None, good, 2, br.SLOPE, dW.ptr(), db.ptr(), 0, nat.ptr(ws), st)
    torch.cuda.synchronize()
    assert rc != 0 and gx.all_untouched() and dW.untouched() and db.untouched() and bng.untouched(), "MODE 1 backward without " + what


@pytest.mark.parametrize("geom", [tr.GEOMS[5], tr.GEOMS[10], tr.GEOMS[11]], ids=tr.geom_id)
def test_backward_is_deterministic(geom):
  """the same MODE 1 launch twice: identical bits in g_x, dW, db, bn_grads and sums_next"""
  B, H, W, groups, _ = geom
  g = _pcl(geom)
  c = tr.bwd_case("zero_mean", geom)
  w, _ = tr.random_weights(3)
  st, st_t = tr.craft_state(c["z"], c["gamma"], groups, c["beta"])
  stn, stn_t = tr.craft_state(c["z_next"], c["gamma_next"], groups, c["beta_next"])
  xb, zb, znb = PclBuf(g, c["x"]), PclBuf(g, c["z"]), PclBuf(g, c["z_next"])
  gab, above = _sums_by_mode0(g, groups, c["g_a"], zb, st_t, xb)
  runs = []
  for _ in range(2):
    b = Bwd(g, groups, gab, xb, w, z=zb, state=st_t, sums=above.sums_next.view, nparts=above.parts, gamma=c["gamma"], z_next=znb,
            state_next=stn_t)
    torch.cuda.synchronize()
    runs.append([b.g_x.raw.clone(), b.dW.buf.clone(), b.db.buf.clone(), b.bn_grads.buf.clone(), b.sums_next.buf.clone()])
  for name, p, q in zip(("g_x", "dW", "db", "bn_grads", "sums_next"), runs[0], runs[1]):
    assert torch.equal(p, q), "%s differs between two identical launches" % name
