"""The middle of the cost-aggregation chain, the four 3x3x3 32 -> 32 layers, through the C ABI, ONE LAUNCH AT A TIME, against the
float64 restatements and the derived bounds of tests/agg_ref.py (held to torch on the CPU, and shown to discriminate, by
tests/test_agg_ref_cpu.py): as_agg3d_fwd in its five flavours (raw + moments, the previous BatchNorm as an affine with and without
the by-product, that BatchNorm still in partials, the eval epilogue, the data gradient) in the contiguous and the column-strip
form, as_conv32_fwd on conv3d_lds_kernel and as_conv32_wgrad on conv3d_wgrad_lds_kernel + the slab reduction, at the smallest
shapes that reach each path: one unit on a grid of 8, D = 1 and 2, Wp = 34 and 83, ragged segments of 2 and 4 planes, a second
round of 256 units, strips with and without overlap columns, Wp = 191 against 192, the cap of 168 slabs, full rounds, extra tiles
and padding chunks of the weight gradient.

Every case first asserts its route through the read-only queries (as_agg3d_ok, as_agg3d_parts, as_agg3d_plan,
as_conv32_stat_parts, as_conv32_wgrad_segments, as_conv32_wgrad_workspace, as_conv3d_wgrad_lds_assignment) against the Python
restatement of the host code: every plan gives equal outputs by design, so nothing else could tell which one ran.

Outputs, their halos and the slab workspace start as one NaN bit pattern between guard words; inputs sit between guard words with
their halo zeroed.  Every interior element must be overwritten and is judged; none is left out.  a_out's halo must keep the
pattern.  The halo of z and g_x may hold +0.0 exactly where agg3d.hip stores its zeros — the halo columns between the rows a
tile's 128 positions span (contiguous form), voxel 0 of a plane (strip form) — and must keep the pattern everywhere else: the halo
planes, the pad rows beyond a tile's span, the guards.  The random family runs once more onto zero-initialised outputs: the whole
halo must then be exactly zero (the production contract) and the interior the same bits.  Single-tap weights (27 taps), the
small-integer family and the two-impulse weight gradients are bit-exact over the whole tensor.  Moments are judged in
tests/test_gpu_batchnorm_fp64.py; here every partial's count must equal the restated ownership of its unit (idle workgroups:
(0, 0, 0)).  The worst err / bound of every entry point goes to conftest.parity_note (agg3d[...]).

Worst err / bound seen on an MI355X, per entry point:
  as_agg3d_fwd     z 0.048 (3 x 5 x 9 x 40; affine operand 0.053, operand in partials 0.017), a_out 0.33 (both operand forms),
                   y of the eval epilogue 0.048, g_x 0.049 (2 x 3 x 5 x 32); the state published from the partials: mean 0.50,
                   invstd 0.50, scale 0.48, shift 0.49, running_mean 0.50, running_var 0.38 (one ulp of the result is most of
                   bn_ref.merge_bounds: half of it is as tight as a correctly rounded result gets)
  as_conv32_fwd    z 0.048 and y 0.048 on conv3d_lds_kernel (3 x 5 x 9 x 40), 0.015 on the generic kernel at Wp = 192
  as_conv32_wgrad  dW 0.083 and db 0.014 on 1 x 1 x 2 x 63 (accumulate 0.080 and 0.016); 0.028 at Wp = 191, 0.031 on the generic
                   kernel at Wp = 192; below 1e-3 from 167 tiles up
Every single-tap, integer and two-impulse case was bit-exact, as_agg3d_fwd gave conv3d_lds_kernel's bits wherever both apply,
every partial counted the voxels of its unit.  No defect found in the kernels.  The file takes 12 s (the slowest case, 257 x 1 x
2 x 63, 3.7 s, most of it the float64 reference).
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from adaptive_stereo import _native as nat
from adaptive_stereo import hip_ops as ops
from adaptive_stereo.hip_ops import Pcl, CONV3D_333
import agg_ref as ar
from conftest import parity_note
from test_gpu_tail_fp64 import PclBuf, Flat, PATTERN, GUARD, _dev

DEV = "cuda:0"
SLOPE = 0.2
SHAPE = CONV3D_333


# ----------------------------------------------------------------------------- judging
class Worst(object):
  def __init__(self, tag):
    self.tag, self.r = tag, {}

  def inside(self, name, got, ref, bound):
    got, ref, bound = got.double().reshape(ref.shape), ref.double(), bound.double().reshape(ref.shape)
    r = ar.ratio(got, ref, bound)
    self.r[name] = max(self.r.get(name, 0.0), r)
    print("  agg3d[%s] %s err/bound %.4f" % (self.tag, name, r))
    if not r <= 1.0:
      q = ((got - ref).abs() / bound.clamp(min=1e-300)).nan_to_num(float("inf")).reshape(-1)
      q = torch.where((got - ref).abs().reshape(-1) == 0, torch.zeros_like(q), q)
      i = int(q.argmax())
      raise AssertionError("%s: %s err/bound %.3g at flat index %d (got %r, reference %r, bound %.3e), %d of %d elements over" % (
          self.tag, name, r, i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(bound.reshape(-1)[i]),
          int((q > 1).sum()), q.numel()))

  def exact(self, name, got, ref):
    got, ref = got.double().reshape(ref.shape), ref.double()
    assert bool(torch.equal(got, ref)), "%s: %s differs from the exact result in %d of %d elements (largest difference %.3e)" % (
        self.tag, name, int((got != ref).sum()), ref.numel(), float((got - ref).abs().nan_to_num(float("inf")).max()))

  def note(self, **extra):
    parity_note("agg3d[%s]" % self.tag, **extra, **{"worst_err_over_bound_" + k: round(v, 4) for k, v in self.r.items()})


def _out(g, zero=False):
  """an output of geometry g: PATTERN everywhere, or (the production contract) zeros everywhere"""
  B, D, H, W = g.B, g.D, g.H, g.W
  return PclBuf(g, torch.zeros(B, D, H, W, 32), "zero") if zero else PclBuf(g, None, "pattern")


def _read(buf, geom, what, halo_zero=None):
  """The interior [B, D, H, W, 32] of an output that started as PATTERN: guards kept, every interior element written, every halo
  word still the pattern — except, where halo_zero ([H + 2, W + 2], planes 1 .. D) allows a stored zero, the pattern or +0.0.
  Returns (interior, halo words that hold a zero)."""
  torch.cuda.synchronize()
  B, D, H, W = geom
  r = buf.raw.cpu()
  assert bool((r[:GUARD] == PATTERN).all()) and bool((r[-GUARD:] == PATTERN).all()), "%s: wrote outside the tensor" % what
  v = r[GUARD:-GUARD].view(B, D + 2, H + 2, W + 2, 32)
  inner = v[:, 1:1 + D, 1:1 + H, 1:1 + W].contiguous().view(torch.float32)
  assert not bool(torch.isnan(inner).any()), "%s: %d interior elements are NaN (not written, or a guard value was consumed)" % (
      what, int(torch.isnan(inner).sum()))
  halo = v.clone()
  halo[:, 1:1 + D, 1:1 + H, 1:1 + W] = PATTERN
  may = torch.zeros(B, D + 2, H + 2, W + 2, 1, dtype=torch.bool)
  if halo_zero is not None:
    may[:, 1:1 + D] = torch.from_numpy(halo_zero).reshape(1, 1, H + 2, W + 2, 1)
  bad = (halo != PATTERN) & ~(may & (halo == 0))
  assert not bool(bad.any()), "%s: %d halo words hold something else than the pattern (or, where the kernel stores zeros, +0.0)" % (
      what, int(bad.sum()))
  return inner, int((halo == 0).sum())


def _read_zeroed(buf, geom, what, same_as):
  """an output that started as zeros: the whole halo exactly zero, the interior the bits of the run onto the pattern"""
  torch.cuda.synchronize()
  B, D, H, W = geom
  r = buf.raw.cpu()
  assert bool((r[:GUARD] == PATTERN).all()) and bool((r[-GUARD:] == PATTERN).all()), "%s: wrote outside the tensor" % what
  v = r[GUARD:-GUARD].view(B, D + 2, H + 2, W + 2, 32).clone()
  inner = v[:, 1:1 + D, 1:1 + H, 1:1 + W].contiguous().view(torch.float32)
  assert bool(torch.equal(inner.view(torch.int32), same_as.view(torch.int32))), "%s: differs from the run onto the pattern" % what
  v[:, 1:1 + D, 1:1 + H, 1:1 + W] = 0
  assert bool((v == 0).all()), "%s: %d halo words are not +0.0" % (what, int((v != 0).sum()))


class Stats(object):
  """BatchNorm partials of `parts` workgroups, every word PATTERN"""

  def __init__(self, parts):
    self.parts = parts
    self.mean, self.m2, self.cnt = Flat(parts * 32), Flat(parts * 32), Flat(parts)

  def ptrs(self):
    return self.mean.ptr(), self.m2.ptr(), self.cnt.ptr()

  def read(self, what):
    return (self.cnt.result(what + " counts").double(), self.mean.result(what + " means").view(self.parts, 32).double(),
            self.m2.result(what + " M2").view(self.parts, 32).double())


def _agg(x, g, wp, bias, z, scale=None, shift=None, in_bn=None, a_out=None, epilogue=0, ep_scale=None, ep_shift=None, stats=None):
  sm, s2, sc = stats.ptrs() if stats is not None else (None, None, None)
  nat.call("as_agg3d_fwd", x.ptr(), g, nat.ptr(wp), nat.ptr(bias), nat.ptr(scale), nat.ptr(shift), in_bn, a_out.ptr() if a_out is not None else None,
           z.ptr(), int(epilogue), nat.ptr(ep_scale), nat.ptr(ep_shift), SLOPE, sm, s2, sc, nat.stream())
  return z


def _pack(w, transposed=False):
  return ops.pack_weights(w.float().contiguous().to(DEV), SHAPE, transposed)


def _assert_agg_route(geom, expect):
  """as_agg3d_ok, as_agg3d_parts and as_agg3d_plan against the restated plan; returns it"""
  lib = nat.load()
  g = Pcl(*geom, 1, 1, 1)
  p = ar.agg_plan(geom)
  out = (ctypes.c_int * 8)()
  assert p is not None and lib.as_agg3d_ok(g) == 1
  assert lib.as_agg3d_plan(g, out) == 1 and list(out) == ar.plan_vector(p), (geom, list(out), p)
  assert lib.as_agg3d_parts(g) == p["grid"] == 8 * p["per_xcd"]
  for k, v in expect.items():
    got = ar.strip_origin(p, geom[3], p["strips"] - 1)[1] if k == "dupc" else p[k]
    assert got == v, (geom, k, got, v)
  return g, p


def _check_counts(wt, geom, p, stats, what):
  cnt, mean, m2 = stats.read(what)
  B, D, H, W = geom
  exp = ar.partial_counts(geom).double()
  assert float(cnt.sum()) == B * D * H * W, "%s: the partials count %r voxels of %d" % (what, float(cnt.sum()), B * D * H * W)
  assert bool(torch.equal(cnt, exp)), "%s: %d partials do not count the voxels their unit owns" % (what, int((cnt != exp).sum()))
  idle = exp == 0
  assert int(idle.sum()) == p["grid"] - p["units"]
  assert float(mean[idle].abs().max() if bool(idle.any()) else 0.0) == 0.0 and float(m2[idle].abs().max() if bool(idle.any()) else 0.0) == 0.0, \
      "%s: an idle workgroup's partial is not (0, 0, 0)" % what
  return cnt, mean, m2


# ----------------------------------------------------------------------------- as_agg3d_fwd
AGG_ALL = [(g, e) for g, e in ar.AGG_GEOMS] + [(g, e) for g, e in ar.STRIP_GEOMS]


@pytest.mark.parametrize("geom,expect", AGG_ALL, ids=[ar.geom_id(g) for g, _ in AGG_ALL])
def test_agg3d_five_flavours(geom, expect):
  """as_agg3d_fwd, the random family with sentinels, in all five launch flavours; the contiguous form from one unit on a grid of 8
  to a second round of 256, the strip form with two and three strips, every one with a shifted-back last tile"""
  g, p = _assert_agg_route(geom, expect)
  B, D, H, W = geom
  tiles = ar.plane_tiles(geom)
  hz = tiles["halo_zero"]
  wt = Worst("%s %s" % (ar.geom_id(geom), "strips" if p["strips"] > 1 else "contiguous"))
  c = ar.random_case(geom)
  x_buf, g_buf = PclBuf(g, c["x"]), PclBuf(g, c["g"])
  wp, wpt, bd = _pack(c["w"]), _pack(c["w"], True), _dev(c["b"])
  sc, sh = _dev(c["scale"]), _dev(c["shift"])

  # 1. raw + moments (layer 1), onto the pattern and onto zeros
  ref = ar.forward(c["x"], c["w"], c["b"], ep_scale=c["scale"], ep_shift=c["shift"])
  st1 = Stats(p["grid"])
  z1, nz = _read(_agg(x_buf, g, wp, bd, _out(g), stats=st1), geom, "raw + moments", hz)
  wt.inside("z", z1, ref["z"], ref["e_z"])
  cnt, mean, m2 = _check_counts(wt, geom, p, st1, "raw + moments")
  _read_zeroed(_agg(x_buf, g, wp, bd, _out(g, True), stats=Stats(p["grid"])), geom, "raw + moments onto zeros", z1)

  # 2. the eval epilogue
  y, _ = _read(_agg(x_buf, g, wp, bd, _out(g), epilogue=1, ep_scale=sc, ep_shift=sh), geom, "eval epilogue", hz)
  wt.inside("y (eval epilogue)", y, ref["y"], ref["e_y"])
  _read_zeroed(_agg(x_buf, g, wp, bd, _out(g, True), epilogue=1, ep_scale=sc, ep_shift=sh), geom, "eval epilogue onto zeros", y)

  # 3. the data gradient: the transposed packing, no bias, no moments
  dg = ar.data_gradient(c["g"], c["w"])
  gx, _ = _read(_agg(g_buf, g, wpt, None, _out(g), epilogue=2), geom, "data gradient", hz)
  wt.inside("g_x", gx, dg["g_x"], dg["e_g_x"])
  _read_zeroed(_agg(g_buf, g, wpt, None, _out(g, True), epilogue=2), geom, "data gradient onto zeros", gx)

  # 4. the previous BatchNorm as an affine, with and without the by-product (its own buffer: it must not alias the input)
  ra = ar.forward(c["x"], c["w"], c["b"], c["scale"], c["shift"])
  a_out = _out(g)
  z_a = _agg(x_buf, g, wp, bd, _out(g), scale=sc, shift=sh, a_out=a_out, stats=Stats(p["grid"]))
  za, _ = _read(z_a, geom, "affine operand", hz)
  wt.inside("z (affine operand)", za, ra["z"], ra["e_z"])
  wt.inside("a_out (affine operand)", a_out.interior("a_out (affine operand)"), ra["a"], ra["e_a_out"])
  z_n = _agg(x_buf, g, wp, bd, _out(g), scale=sc, shift=sh)
  torch.cuda.synchronize()
  assert bool(torch.equal(z_n.raw, z_a.raw)), "affine operand without the by-product: %d words differ" % int((z_n.raw != z_a.raw).sum())
  _read_zeroed(_agg(x_buf, g, wp, bd, _out(g, True), scale=sc, shift=sh), geom, "affine operand onto zeros", za)

  # 5. layer 2 on layer 1's partials: every workgroup merges them, workgroup 0 publishes the state
  z1_buf = PclBuf(g, z1)
  gam, bet = _dev(c["gamma"]), _dev(c["beta"])
  rm, rv = Flat(32, c["rm"]), Flat(32, c["rv"])
  pub = [Flat(32) for _ in range(4)]                       # mean, invstd, scale, shift
  block = nat.BnMerge(st1.mean.ptr(), st1.m2.ptr(), st1.cnt.ptr(), nat.ptr(gam), nat.ptr(bet), rm.ptr(), rv.ptr(), pub[0].ptr(),
                      pub[1].ptr(), pub[2].ptr(), pub[3].ptr(), p["grid"], 0.1, 1e-5)
  a2, st2 = _out(g), Stats(p["grid"])
  z2, _ = _read(_agg(z1_buf, g, wp, bd, _out(g), in_bn=block, a_out=a2, stats=st2), geom, "operand in partials", hz)
  state, e_state = ar.merged_state(cnt, mean, m2, c["gamma"], c["beta"], c["rm"], c["rv"])
  got = dict(mean=pub[0].result("published mean"), invstd=pub[1].result("published invstd"), scale=pub[2].result("published scale"),
             shift=pub[3].result("published shift"), running_mean=rm.result("running_mean"), running_var=rv.result("running_var"))
  for f in sorted(got):
    wt.inside("merge " + f, got[f], state[f], e_state[f])
  rp = ar.forward(z1, c["w"], c["b"], got["scale"], got["shift"])
  wt.inside("a_out (operand in partials)", a2.interior("a_out (operand in partials)"), rp["a"], rp["e_a_out"])
  wt.inside("z (operand in partials)", z2, rp["z"], rp["e_z"])
  _check_counts(wt, geom, p, st2, "operand in partials")
  wt.note(units=p["units"], grid=p["grid"], seg_len=p["seg_len"], strips=p["strips"], halo_zero_words=nz)


@pytest.mark.parametrize("geom", ar.EXACT_GEOMS, ids=ar.geom_id)
def test_agg3d_exact_families(geom):
  """27 single-tap weights (forward and data gradient are copies scaled by a power of two, bias 0) and the small-integer family
  (every sum a whole number below 2^24): bit-exact over the whole tensor"""
  expect = dict(ar.AGG_GEOMS + ar.STRIP_GEOMS)[geom]
  g, p = _assert_agg_route(geom, expect)
  hz = ar.plane_tiles(geom)["halo_zero"]
  wt = Worst("%s exact" % ar.geom_id(geom))
  c = ar.random_case(geom)
  x_buf, g_buf = PclBuf(g, c["x"]), PclBuf(g, c["g"])
  zero_bias = torch.zeros(32, device=DEV)
  for t in range(27):
    w = ar.tap_weights(t)
    z, _ = _read(_agg(x_buf, g, _pack(w), zero_bias, _out(g), stats=Stats(p["grid"])), geom, "single tap %d" % t, hz)
    wt.exact("z single tap %d" % t, z, ar.conv_sum(ar.pad_operand(c["x"]), w))
    gx, _ = _read(_agg(g_buf, g, _pack(w, True), None, _out(g), epilogue=2), geom, "data gradient, single tap %d" % t, hz)
    wt.exact("g_x single tap %d" % t, gx, ar.conv_sum(ar.pad_operand(c["g"]), ar.transposed(w)))
  i = ar.integer_case(geom)
  xi, gi = PclBuf(g, i["x"]), PclBuf(g, i["g"])
  z, _ = _read(_agg(xi, g, _pack(i["w"]), _dev(i["b"]), _out(g), stats=Stats(p["grid"])), geom, "integers", hz)
  wt.exact("z integers", z, ar.conv_sum(ar.pad_operand(i["x"]), i["w"], i["b"]))
  gx, _ = _read(_agg(gi, g, _pack(i["w"], True), None, _out(g), epilogue=2), geom, "data gradient, integers", hz)
  wt.exact("g_x integers", gx, ar.conv_sum(ar.pad_operand(i["g"]), ar.transposed(i["w"])))
  wt.note(units=p["units"])


# ----------------------------------------------------------------------------- as_conv32_fwd on the 3-D LDS route
def _conv32(x, g, wp, bias, z, epilogue=0, ep_scale=None, ep_shift=None, stats=None):
  sm, s2, sc = stats.ptrs() if stats is not None else (None, None, None)
  nat.call("as_conv32_fwd", x.ptr(), g, nat.ptr(wp), nat.ptr(bias), z.ptr(), g, SHAPE, int(epilogue), nat.ptr(ep_scale), nat.ptr(ep_shift),
           SLOPE, None, sm, s2, sc, nat.stream())
  return z


@pytest.mark.parametrize("geom,lds", ar.FIRST_GEN_GEOMS, ids=[ar.geom_id(g) for g, _ in ar.FIRST_GEN_GEOMS])
def test_first_generation_forward(geom, lds):
  """as_conv32_fwd on conv3d_lds_kernel (one tile, the narrowest row, several tiles and planes, Wp = 191: the last width it takes)
  and, at Wp = 192, on whichever kernel takes the layer then: raw + moments and the eval epilogue inside the same bounds; on the
  LDS route bit-equal to as_agg3d_fwd on the same operands"""
  lib = nat.load()
  B, D, H, W = geom
  g = Pcl(B, D, H, W, 1, 1, 1)
  parts = lib.as_conv32_stat_parts(g, g, SHAPE)
  assert ar.lds3d_ok(geom) == lds and parts == ar.stat_parts(geom), (parts, ar.stat_parts(geom))
  assert parts == (B * D * ar.lds3d_tiles_per_plane(geom) if lds else (B * D * H * W + 127) // 128)
  wt = Worst("conv32 %s %s" % (ar.geom_id(geom), "conv3d_lds" if lds else "generic"))
  c = ar.random_case(geom)
  x_buf = PclBuf(g, c["x"])
  wp, bd, sc, sh = _pack(c["w"]), _dev(c["b"]), _dev(c["scale"]), _dev(c["shift"])
  ref = ar.forward(c["x"], c["w"], c["b"], ep_scale=c["scale"], ep_shift=c["shift"])
  st = Stats(parts)
  z_buf = _conv32(x_buf, g, wp, bd, _out(g), stats=st)
  z, _ = _read(z_buf, geom, "as_conv32_fwd raw + moments")               # (no halo word may change: the kernel stores interior voxels only)
  wt.inside("z", z, ref["z"], ref["e_z"])
  cnt = st.read("as_conv32_fwd")[0]
  assert float(cnt.sum()) == B * D * H * W
  y_buf = _conv32(x_buf, g, wp, bd, _out(g), epilogue=1, ep_scale=sc, ep_shift=sh)
  y, _ = _read(y_buf, geom, "as_conv32_fwd eval epilogue")
  wt.inside("y (eval epilogue)", y, ref["y"], ref["e_y"])
  if lds:
    assert lib.as_agg3d_ok(g) == 1
    p = ar.agg_plan(geom)
    z2, _ = _read(_agg(x_buf, g, wp, bd, _out(g), stats=Stats(p["grid"])), geom, "as_agg3d_fwd", ar.plane_tiles(geom)["halo_zero"])
    assert bool(torch.equal(z2.view(torch.int32), z.view(torch.int32))), "as_agg3d_fwd and conv3d_lds_kernel differ in %d elements" % int((z2 != z).sum())
    y2, _ = _read(_agg(x_buf, g, wp, bd, _out(g), epilogue=1, ep_scale=sc, ep_shift=sh), geom, "as_agg3d_fwd eval", ar.plane_tiles(geom)["halo_zero"])
    assert bool(torch.equal(y2.view(torch.int32), y.view(torch.int32))), "eval epilogue: as_agg3d_fwd and conv3d_lds_kernel differ"
  wt.note(parts=parts)


# ----------------------------------------------------------------------------- as_conv32_wgrad on the 3-D LDS route
def _wgrad(x_buf, g_buf, g, plan, d0=None, b0=None):
  ws = Flat(plan["workspace"])
  dW, db = Flat(32 * 32 * 27, d0), Flat(32, b0)
  nat.call("as_conv32_wgrad", x_buf.ptr(), g, g_buf.ptr(), g, SHAPE, dW.ptr(), db.ptr(), 1 if d0 is not None else 0, ws.ptr(), nat.stream())
  # (no deferral region is open: the slab reduction is enqueued behind the kernel; result() synchronizes before it reads)
  ws.guards_kept("as_conv32_wgrad workspace")
  return dW.result("as_conv32_wgrad dW").view(32, 32, 3, 3, 3), db.result("as_conv32_wgrad db")


@pytest.mark.parametrize("geom,expect", ar.WGRAD_GEOMS, ids=[ar.geom_id(g) for g, _ in ar.WGRAD_GEOMS])
def test_weight_gradient(geom, expect):
  """as_conv32_wgrad on conv3d_wgrad_lds_kernel + the slab reduction: one chunk and seven padding chunks, per_xcd 2, a ragged
  unshifted last tile with clamped DMA groups, either side of the cap of 168 slabs, full rounds with extra tiles, Wp = 191 — and
  Wp = 192 on the generic kernel; accumulate 0 and 1 on the first and the last geometry"""
  lib = nat.load()
  B, D, H, W = geom
  g = Pcl(B, D, H, W, 1, 1, 1)
  plan = ar.wgrad_plan(geom)
  assert (plan["tiles"], plan["slabs"] if plan["lds"] else 0) == expect
  assert lib.as_conv32_wgrad_segments(g, g, SHAPE) == plan["segments"] and (plan["segments"] == 0) == plan["lds"]
  assert lib.as_conv32_wgrad_workspace(g, g, SHAPE) == plan["workspace"]
  if plan["lds"]:
    ci, ki, ei = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for blk in range(ar.wgrad_grid(plan["slabs"])):
      ok = lib.as_conv3d_wgrad_lds_assignment(plan["tiles"], plan["slabs"], blk, ctypes.byref(ci), ctypes.byref(ki), ctypes.byref(ei))
      exp = ar.wgrad_assign(blk, plan["tiles"], plan["slabs"])
      assert (bool(ok), ki.value, ei.value) == (exp[0], exp[2], exp[3]) and (not ok or ci.value == exp[1]), blk
    assert bool((ar.wgrad_coverage(plan["tiles"], plan["slabs"]) == 1).all())
  wt = Worst("wgrad %s %s" % (ar.geom_id(geom), "%d tiles in %d slabs" % expect if plan["lds"] else "generic"))
  both = geom in (ar.WGRAD_GEOMS[0][0], ar.WGRAD_GEOMS[-1][0])
  c = ar.random_case(geom)
  x_buf, g_buf = PclBuf(g, c["x"]), PclBuf(g, c["g"])
  for acc in ((0, 1) if both else (0,)):
    d0, b0 = ar.prior(False) if acc else (None, None)
    ref = ar.weight_gradient(c["x"], c["g"], d0, b0)
    dW, db = _wgrad(x_buf, g_buf, g, plan, d0, b0)
    tag = " accumulate" if acc else ""
    wt.inside("dW" + tag, dW, ref["dW"], ref["e_dW"])
    wt.inside("db" + tag, db, ref["db"], ref["e_db"])
  if geom in ar.WGRAD_EXACT_GEOMS:
    fams = [("integers", ar.integer_case(geom))] + [("two impulses, %s" % s, ar.impulse_case(geom, s)) for s in ar.IMPULSE_SPOTS]
    for k, (name, e) in enumerate(fams):
      acc = k % 2 if both else 0
      d0, b0 = ar.prior(True) if acc else (None, None)
      ref = ar.weight_gradient(e["x"], e["g"], d0, b0)
      dW, db = _wgrad(PclBuf(g, e["x"]), PclBuf(g, e["g"]), g, plan, d0, b0)
      wt.exact("dW %s%s" % (name, " accumulate" if acc else ""), dW, ref["dW"])
      wt.exact("db %s%s" % (name, " accumulate" if acc else ""), db, ref["db"])
  wt.note(tiles=plan["tiles"], slabs=plan["slabs"])
