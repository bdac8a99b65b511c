"""The feature head's 5x5 stride-2 layers through the C ABI, ONE LAUNCH AT A TIME, against the float64 restatement and the derived
bounds of tests/head_ref.py (held to torch on the CPU, and shown to discriminate, by tests/test_head_ref_cpu.py): as_conv4_fwd /
as_conv4_wgrad (the 3 -> 32 first layer), as_conv32_fwd, as_conv32_dgrad_s2 (+ _pack, _packed) and as_conv32_wgrad (the 32 -> 32
layers), at the smallest shapes that reach each route and each side of each route's threshold.  The dispatch counts tiles, not
pixels: many short narrow images reach every kernel with a few MB.

Every case first asserts its route through the read-only queries (as_conv4_s2_ok, as_conv32_s2_fwd_ok, as_conv32_s2_dgrad_ok,
as_conv32_wgrad_segments, as_conv32_stat_parts) — the routes give equal bits by design, so nothing else could tell which kernel
ran — and where the enable switches offer a second route for the same shape, the two outputs must be equal bit for bit.

Outputs and their halos start as one NaN bit pattern: every interior voxel must be overwritten, every halo word must keep the
pattern.  Inputs sit between guard floats of the same pattern inside a larger allocation, their halos zeroed: a value consumed
from outside the padded tensor shows up as NaN (consumption, not the read itself, is what can be seen).  Every geometry runs the
random family with sentinels of +-1e4 on the first and last rows and columns; the smallest geometry of each route also runs all
25 single-tap cases (forward and data gradient are then copies: bit-exact), and the weight gradient the two-impulse cases
(every entry a sum of two exact products: bit-exact).  No element is left out of a comparison; the worst err / bound of every
entry point goes to conftest.parity_note (head[...]).

Worst err / bound seen on an MI355X: first layer z 0.17, dW 0.099 and db 0.057 (both on 1 x 9 x 13; below 1e-4 on the 4096-tile
shapes); 32 -> 32 forward z 0.049 (split-K 0.025); data gradient 0.15; weight gradient dW 0.15 and db 0.062 on 1 x 9 x 13 (8e-4
from 2 x 94 x 311 up), with accumulate 0.13 and 0.051.  Every single-tap and two-impulse case was bit-exact, every pair of
routes gave equal bits.  The file takes 7 s.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from adaptive_stereo import _native as nat
from adaptive_stereo import hip_ops as ops
from adaptive_stereo.hip_ops import Pcl, ConvShape
import head_ref as hr
from conftest import parity_note

DEV = "cuda:0"
PATTERN = 0x7FF92345        # a quiet NaN that no arithmetic produces
GUARD = 64
SHAPE = ConvShape(1, 5, 5, 0, 2, 2, 1, 2)
ALL_TAPS = [("tap", t) for t in range(25)]


# ----------------------------------------------------------------------------- buffers
class OutBuf(object):
  """an output with a halo (PCL: [B, H + 2 ph, W + 2 pw, 32]), every word PATTERN"""

  def __init__(self, g):
    self.g = g
    self.raw = torch.full((GUARD + g.numel() + GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    self.body = self.raw[GUARD:GUARD + g.numel()]

  def ptr(self):
    return nat.ptr(self.body)

  def interior(self, what):
    torch.cuda.synchronize()
    g = self.g
    r = self.raw.cpu()
    assert bool((r[:GUARD] == PATTERN).all()) and bool((r[-GUARD:] == PATTERN).all()), "%s: wrote outside the tensor" % what
    v = r[GUARD:-GUARD].view(g.B, g.H + 2 * g.ph, g.W + 2 * g.pw, 32)
    inner = v[:, g.ph:g.ph + g.H, g.pw:g.pw + g.W].contiguous()
    halo = v.clone()
    halo[:, g.ph:g.ph + g.H, g.pw:g.pw + g.W] = PATTERN
    assert bool((halo == PATTERN).all()), "%s: %d halo words were written" % (what, int((halo != PATTERN).sum()))
    f = inner.view(torch.float32)
    assert not bool(torch.isnan(f).any()), "%s: %d interior elements are NaN (not written, or a guard value was consumed)" % (
        what, int(torch.isnan(f).sum()))
    return f


class InBuf(object):
  """a channel-last input [B, H, W, C] inside a zero halo (ph, pw), between guard floats of PATTERN"""

  def __init__(self, t, ph, pw, cpad=0):
    p = F.pad(t.float(), (0, cpad, pw, pw, ph, ph)).contiguous().reshape(-1)
    self.raw = torch.full((GUARD + p.numel() + GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    self.body = self.raw[GUARD:GUARD + p.numel()].view(torch.float32)
    self.body.copy_(p.to(DEV))

  def ptr(self):
    return nat.ptr(self.body)


class Flat(object):
  """numel fp32 outputs inside a buffer of PATTERN; `init` for an accumulating launch"""

  def __init__(self, numel, init=None):
    self.raw = torch.full((GUARD + numel + GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    self.body = self.raw[GUARD:GUARD + numel].view(torch.float32)
    if init is not None:
      self.body.copy_(init.reshape(-1).to(DEV))

  def ptr(self):
    return nat.ptr(self.body)

  def result(self, what):
    torch.cuda.synchronize()
    r = self.raw.cpu()
    assert bool((r[:GUARD] == PATTERN).all()) and bool((r[-GUARD:] == PATTERN).all()), "%s: wrote outside the destination" % what
    v = r[GUARD:-GUARD].view(torch.float32)
    assert not bool(torch.isnan(v).any()), "%s: %d elements not written" % (what, int(torch.isnan(v).sum()))
    return v


class Worst(object):
  def __init__(self, tag):
    self.tag, self.r = tag, {}

  def inside(self, name, got, ref, bound):
    got, ref, bound = got.double().reshape(ref.shape), ref.double(), bound.double().reshape(ref.shape)
    r = hr.ratio(got, ref, bound)
    self.r[name] = max(self.r.get(name, 0.0), r)
    if not r <= 1.0:
      q = ((got - ref).abs() / bound.clamp(min=1e-300)).nan_to_num(float("inf")).reshape(-1)
      i = int(q.argmax())
      raise AssertionError("%s: %s err/bound %.3g at flat index %d (got %r, reference %r, bound %.3e), %d of %d elements over" % (
          self.tag, name, r, i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(bound.reshape(-1)[i]),
          int((q > 1).sum()), q.numel()))

  def exact(self, name, got, ref):
    got, ref = got.double().reshape(ref.shape), ref.double()
    assert bool(torch.equal(got, ref)), "%s: %s differs from the exact result in %d of %d elements (largest difference %.3e)" % (
        self.tag, name, int((got != ref).sum()), ref.numel(), float((got - ref).abs().nan_to_num(float("inf")).max()))

  def note(self, **extra):
    parity_note("head[%s]" % self.tag, **extra, **{"worst_err_over_bound_" + k: v for k, v in self.r.items()})


class Switch(object):
  """an enable switch of the library set for the duration, restored after"""

  def __init__(self, name, on):
    self.name, self.on = name, on

  def __enter__(self):
    self.prev = getattr(nat.load(), self.name)(2)
    getattr(nat.load(), self.name)(self.on)

  def __exit__(self, *exc):
    getattr(nat.load(), self.name)(self.prev)


def _out_geom(geom, halo):
  B, H, W = geom
  return Pcl(B, 1, hr.out_extent(H), hr.out_extent(W), 0, halo, halo)


def _tiles(g):
  return g.B * g.H * ((g.W + 31) // 32)


# ----------------------------------------------------------------------------- the first layer
def _conv4_fwd(x_in, g4, wp, bias, gout):
  z = OutBuf(gout)
  nat.call("as_conv4_fwd", x_in.ptr(), g4, nat.ptr(wp), nat.ptr(bias), z.ptr(), gout, SHAPE, 0, None, None, 0.2, None, None, None,
           nat.stream())
  return z


def _pack4(w):
  wp = torch.empty(25 * 128, device=DEV)
  wd = w.to(DEV)
  nat.call("as_conv4_pack_weights", nat.ptr(wd), 3, nat.ptr(wp), SHAPE, nat.stream())
  return wp


SMALLEST_CONV4 = {(64, 127, 63), (1, 9, 13)}


@pytest.mark.parametrize("geom,staged", hr.CONV4_GEOMS, ids=[hr.geom_id(g) for g, _ in hr.CONV4_GEOMS])
def test_first_layer_forward_and_weight_gradient(geom, staged):
  """as_conv4_fwd (plain epilogue) and as_conv4_wgrad of Conv2d(3, 32, 5, stride 2, padding 2): conv4_s2_fwd_kernel from 4096 tiles
  (the threshold exactly, odd / odd and even / even, a one-column second segment, a ragged last round of the persistent waves),
  conv4_fwd_kernel<25> below; conv4_s2_wgrad_kernel at every size."""
  lib = nat.load()
  B, H, W = geom
  g4, gout = Pcl(B, 1, H, W, 0, 2, 2), _out_geom(geom, 2)
  assert lib.as_conv4_s2_enable(2) == 1
  assert lib.as_conv4_s2_ok(g4, gout, SHAPE) == staged == (1 if _tiles(gout) >= 4096 else 0), (_tiles(gout), staged)
  wt = Worst("conv4 %s %s" % (hr.geom_id(geom), "staged rows" if staged else "one tile"))
  fams = ["random"] + (ALL_TAPS if geom in SMALLEST_CONV4 else [])
  x_in = None
  for fam in fams:
    c = hr.fwd_case(geom, fam, 3)
    x_in = x_in or InBuf(c["x"], 2, 2, cpad=1)               # (the same x in every family)
    wp, bd = _pack4(c["w"]), c["b"].to(DEV)
    z = _conv4_fwd(x_in, g4, wp, bd, gout)
    got = z.interior("as_conv4_fwd %s" % (fam,))
    if fam == "random":
      ref = hr.forward(c["x"], c["w"], c["b"])
      wt.inside("z", got, ref["z"], ref["e_z"])
    else:
      wt.exact("z single tap %d" % fam[1], got, hr.fwd_sum(c["x"], c["w"], c["b"]))
    if staged and (fam == "random" or fam[1] % 6 == 0):
      with Switch("as_conv4_s2_enable", 0):
        assert lib.as_conv4_s2_ok(g4, gout, SHAPE) == 0
        z0 = _conv4_fwd(x_in, g4, wp, bd, gout)
        torch.cuda.synchronize()
      assert bool(torch.equal(z0.raw, z.raw)), "staged rows and the one-tile kernel differ in %d words" % int((z0.raw != z.raw).sum())
  # the weight gradient on the same shape
  # (its units are 64 output pixels of a row, 32 pair-steps: the seam of a row of 66 lies between columns 63 and 64)
  for fam in ["random"] + [("impulse", s) for s in hr.IMPULSE_SPOTS if geom in SMALLEST_CONV4 or gout.W > 64]:
    c = hr.wgrad_case(geom, fam, 3, seam=32 if gout.W > 64 else None)
    xi, gi = InBuf(c["x"], 2, 2, cpad=1), InBuf(c["gz"], 2, 2)
    ws = torch.empty(lib.as_conv4_wgrad_workspace(gout, SHAPE), device=DEV)
    dW, db = Flat(32 * 3 * 25), Flat(32)
    nat.call("as_conv4_wgrad", xi.ptr(), g4, gi.ptr(), gout, SHAPE, 3, dW.ptr(), db.ptr(), 0, nat.ptr(ws), nat.stream())
    ref = hr.weight_gradient(c["x"], c["gz"])
    if fam == "random":
      wt.inside("dW", dW.result("as_conv4_wgrad dW"), ref["dW"], ref["e_dW"])
      wt.inside("db", db.result("as_conv4_wgrad db"), ref["db"], ref["e_db"])
    else:
      wt.exact("dW two impulses %s" % fam[1], dW.result("as_conv4_wgrad dW"), ref["dW"])
      wt.exact("db two impulses %s" % fam[1], db.result("as_conv4_wgrad db"), ref["db"])
  wt.note(tiles=_tiles(gout))


# ----------------------------------------------------------------------------- 32 -> 32 forward
def _conv32_fwd(x_in, gin, wp, bias, gout):
  z = OutBuf(gout)
  nat.call("as_conv32_fwd", x_in.ptr(), gin, nat.ptr(wp), nat.ptr(bias), z.ptr(), gout, SHAPE, 0, None, None, 0.2, None, None,
           None, None, nat.stream())
  return z


SMALLEST_FWD = {(32, 63, 33), (3, 21, 33), (31, 63, 33)}


@pytest.mark.parametrize("geom,route", hr.FWD_GEOMS, ids=["%s-%s" % (hr.geom_id(g), r) for g, r in hr.FWD_GEOMS])
def test_strided_forward(geom, route):
  """as_conv32_fwd (epilogue 0, no residual, no moments) of Conv2d(32, 32, 5, stride 2, padding 2) on each of its three kernels:
  split-K (M <= 16384, which has precedence), staged rows (>= 1024 tiles) and the direct-load kernel, both sides of both
  thresholds; output halo 2 (odd H) and 1 (even H)."""
  lib = nat.load()
  B, H, W = geom
  gin, gout = Pcl(B, 1, H, W, 0, 2, 2), _out_geom(geom, 1 + (H & 1))
  M = gout.B * gout.H * gout.W
  assert lib.as_conv32_s2_enable(2) == 1
  assert lib.as_conv32_s2_fwd_ok(gin, gout, SHAPE) == (1 if route == "staged" else 0), (_tiles(gout), M)
  parts = lib.as_conv32_stat_parts(gin, gout, SHAPE)
  if route == "splitk":
    assert M <= 16384 and parts == (M + 31) // 32
  else:
    assert M > 16384 and parts == lib.as_conv32_num_blocks(gout)
    assert (_tiles(gout) >= 1024) == (route == "staged")
  wt = Worst("conv32 fwd %s %s" % (hr.geom_id(geom), route))
  x_in = None
  for fam in ["random"] + (ALL_TAPS if geom in SMALLEST_FWD else []):
    c = hr.fwd_case(geom, fam)
    x_in = x_in or InBuf(c["x"], 2, 2)
    wp, bd = ops.pack_weights(c["w"].to(DEV), SHAPE, False), c["b"].to(DEV)
    z = _conv32_fwd(x_in, gin, wp, bd, gout)
    got = z.interior("as_conv32_fwd %s" % (fam,))
    if fam == "random":
      ref = hr.forward(c["x"], c["w"], c["b"])
      wt.inside("z", got, ref["z"], ref["e_z"])
    else:
      wt.exact("z single tap %d" % fam[1], got, hr.fwd_sum(c["x"], c["w"], c["b"]))
    if route == "staged" and (fam == "random" or fam[1] % 6 == 0):
      with Switch("as_conv32_s2_enable", 0):
        assert lib.as_conv32_s2_fwd_ok(gin, gout, SHAPE) == 0
        z0 = _conv32_fwd(x_in, gin, wp, bd, gout)
        torch.cuda.synchronize()
      assert bool(torch.equal(z0.raw, z.raw)), "staged rows and the direct-load kernel differ in %d words" % int((z0.raw != z.raw).sum())
  wt.note(tiles=_tiles(gout), M=M)


# ----------------------------------------------------------------------------- 32 -> 32 data gradient
def _dgrad(gz_in, ggz, w_dev, ggx, packed_route):
  gx = OutBuf(ggx)
  ws = torch.empty(nat.load().as_conv32_dgrad_s2_workspace(), device=DEV)
  if packed_route:
    nat.call("as_conv32_dgrad_s2_pack", nat.ptr(w_dev), nat.ptr(ws), nat.stream())
    nat.call("as_conv32_dgrad_s2_packed", gz_in.ptr(), ggz, nat.ptr(ws), gx.ptr(), ggx, nat.stream())
  else:
    nat.call("as_conv32_dgrad_s2", gz_in.ptr(), ggz, nat.ptr(w_dev), gx.ptr(), ggx, nat.ptr(ws), nat.stream())
  return gx


SMALLEST_DGRAD = {(32, 63, 33), (1, 1, 1), (1, 2, 2), (1, 5, 7)}


@pytest.mark.parametrize("geom,staged", hr.DGRAD_GEOMS, ids=[hr.geom_id(g) for g, _ in hr.DGRAD_GEOMS])
def test_strided_data_gradient(geom, staged):
  """as_conv32_dgrad_s2 and as_conv32_dgrad_s2_pack + as_conv32_dgrad_s2_packed (equal bits) on conv32_s2_dgrad_kernel (g_z tiles
  >= 1024) and on the generic four-phase kernel, every parity class of (H, W) on either, degenerate phases; g_z halo 1 and 2."""
  lib = nat.load()
  B, H, W = geom
  ggx = Pcl(B, 1, H, W, 0, 2, 2)
  assert lib.as_conv32_s2_enable(2) == 1
  wt = Worst("conv32 dgrad %s %s" % (hr.geom_id(geom), "staged rows" if staged else "four phases"))
  for fam in ["random"] + (ALL_TAPS if geom in SMALLEST_DGRAD else []):
    c = hr.dgrad_case(geom, fam)
    wd = c["w"].to(DEV)
    if fam == "random":
      ref = hr.data_gradient(c["gz"], c["w"], H, W)
      ref_in = ref["g_x"][:, 1:-1, 1:-1]
    else:
      ref_in = hr.dgrad_sum(c["gz"], c["w"], H, W)[:, 1:-1, 1:-1]
    for pz in ((1, 2) if fam == "random" or fam[1] % 6 == 0 else (1,)):
      ggz = _out_geom(geom, pz)
      assert lib.as_conv32_s2_dgrad_ok(ggz, ggx) == staged == (1 if _tiles(ggz) >= 1024 else 0), _tiles(ggz)
      gz_in = InBuf(c["gz"], pz, pz)
      gx = _dgrad(gz_in, ggz, wd, ggx, False)
      got = gx.interior("as_conv32_dgrad_s2 %s halo %d" % (fam, pz))
      if fam == "random":
        wt.inside("g_x", got, ref_in, ref["e_g_x"])
      else:
        wt.exact("g_x single tap %d" % fam[1], got, ref_in)
      gx2 = _dgrad(gz_in, ggz, wd, ggx, True)
      torch.cuda.synchronize()
      assert bool(torch.equal(gx2.raw, gx.raw)), "as_conv32_dgrad_s2_pack + _packed differ from as_conv32_dgrad_s2"
      if staged:
        with Switch("as_conv32_s2_enable", 0):
          assert lib.as_conv32_s2_dgrad_ok(ggz, ggx) == 0
          gx0 = _dgrad(gz_in, ggz, wd, ggx, False)
          torch.cuda.synchronize()
        assert bool(torch.equal(gx0.raw, gx.raw)), "staged rows and the four-phase kernel differ in %d words" % int((gx0.raw != gx.raw).sum())
  wt.note(tiles=_tiles(_out_geom(geom, 1)))


# ----------------------------------------------------------------------------- 32 -> 32 weight gradient
@pytest.mark.parametrize("geom,nseg", hr.WGRAD_GEOMS, ids=["%s-%dseg" % (hr.geom_id(g), n) for g, n in hr.WGRAD_GEOMS])
def test_strided_weight_gradient(geom, nseg):
  """as_conv32_wgrad on conv32_wgrad_kernel<5> with rows whole and cut into 2 and 3 segments (a ragged last segment, an odd last
  column in a segment other than the first, both sides of the 1024-wave rule), accumulate 0 and 1."""
  lib = nat.load()
  B, H, W = geom
  gin, gout = Pcl(B, 1, H, W, 0, 2, 2), _out_geom(geom, 1 + (H & 1))
  assert lib.as_conv32_wgrad_segments(gin, gout, SHAPE) == nseg
  assert (gout.B * gout.H * 5 < 1024) or nseg == 1
  wt = Worst("conv32 wgrad %s %d segments" % (hr.geom_id(geom), nseg))
  ws = torch.empty(lib.as_conv32_wgrad_workspace(gin, gout, SHAPE), device=DEV)
  for fam in ["random"] + [("impulse", s) for s in hr.IMPULSE_SPOTS]:
    c = hr.wgrad_case(geom, fam, 32, nseg)
    xi, gi = InBuf(c["x"], 2, 2), InBuf(c["gz"], gout.ph, gout.pw)
    for accumulate in (0, 1):
      if accumulate:
        gen = torch.Generator().manual_seed(77)
        d0, b0 = torch.randn(32, 32, 5, 5, generator=gen), torch.randn(32, generator=gen)
        if fam != "random":                                    # (multiples of 2^-8: the sum stays exact)
          d0, b0 = (d0 * 256).round() / 256, (b0 * 256).round() / 256
      else:
        d0 = b0 = None
      dW, db = Flat(32 * 32 * 25, d0), Flat(32, b0)
      nat.call("as_conv32_wgrad", xi.ptr(), gin, gi.ptr(), gout, SHAPE, dW.ptr(), db.ptr(), accumulate, nat.ptr(ws), nat.stream())
      ref = hr.weight_gradient(c["x"], c["gz"], d0, b0)
      tag = " accumulate" if accumulate else ""
      if fam == "random":
        wt.inside("dW" + tag, dW.result("as_conv32_wgrad dW"), ref["dW"], ref["e_dW"])
        wt.inside("db" + tag, db.result("as_conv32_wgrad db"), ref["db"], ref["e_db"])
      else:
        wt.exact("dW two impulses %s%s" % (fam[1], tag), dW.result("as_conv32_wgrad dW"), ref["dW"])
        wt.exact("db two impulses %s%s" % (fam[1], tag), db.result("as_conv32_wgrad db"), ref["db"])
  wt.note(row_waves=gout.B * gout.H * 5)
