"""The two ends of the edge-aware refinement through the C ABI, ONE LAUNCH AT A TIME, against the float64 restatement and the
derived bounds of tests/refine_ends_ref.py (held to torch on the CPU, and shown to tell thirteen mutants from the right
restatement, by tests/test_refine_ends_ref_cpu.py): as_pack_in4, as_conv4_fwd (staged rows and one tile, epilogues 0 / 1 / 2),
as_refine_out_fwd (activation + skip, activation, plain), as_conv32to1_fwd (thin 2-D), as_relu_bwd, as_conv32to1_bwd,
as_conv32to1_dgrad_bnsums, as_mirror_taps_ch0, as_conv4_wgrad, as_conv4_wgrad_bnapply, as_conv4_wgrad_bnapply_proj, as_tap_gather.

Geometries: the lists of refine_ends_ref, each the smallest that reaches an edge of the code — the narrowest staged-row width
of as_conv4_fwd at the production halo (W = 62, every DMA window clamped to slot 0), its 1024-workgroup cap (4134 tiles), the
first width its rows route refuses; the 126-column and 12 / 32-row seams of as_refine_out_fwd, its accepted floor (halo (1, 1),
W = 126: the last staged row ends at the buffer's end) and the refusals; the 14 / 30 patch seams of the thin forward; the
128-voxel chunk seam of the backward kernels, the weight gradients' 1024-workgroup cap (4098 chunks), the data gradient's
16384 cap (16388 chunks) and more chunks than BatchNorm partials (1029).  Every case asserts its route through the read-only
queries before launching.

Buffers: outputs, their halos, slab workspaces and the fp64 partials start as one NaN bit pattern between guard words: every
interior word must be overwritten, every halo and guard word must keep the pattern.  A launch that reads an input halo as a
value (as_conv4_fwd and the conv4 weight gradients: x4; the thin forward: a) gets a zero halo between NaN guards — the thin
forward also once with DATA in the one-voxel border it reads; refine_out_kernel selects zeros outside the image, so its inputs
carry the pattern in their halos, like every input that is read on its interior only.

Families: random with +-1e4 sentinels on the first and last rows and columns of every input; the exact integer family (nine
single-tap weights and a dense one, scale 1, shift 0, slope 1/2, k1 = k2 = 0, k3 = 1) where every output equals float64 bit for
bit.  The float64 references run on the card (the same refine_ends_ref code).  No element is left out except those undecided on
a LeakyReLU branch (g_z, h and the sums), which are counted, capped at 1e-4 of the case and judged against the nearer branch;
into the sums they enter both ways.  The worst err / bound of every output goes to conftest.parity_note (refine_ends[...]).

Worst err / bound seen on an MI355X, random family (every ratio of the 158 cases at most 1, every exact case bit-exact with its
largest accumulator below 2.9e-4 * 2^24 quanta, no element of any case undecided on a LeakyReLU branch):
  as_conv4_fwd           z 0.17 (2 x 5 x 65, x4 halo 2; without bias 0.17 on the one-tile route at 2 x 5 x 61), epilogue 1 0.15
                         (1 x 106 x 1242); z with and without the moments: equal bits everywhere
  as_refine_out_fwd      a_out 0.98 with the skip connection (an element-wise chain with every rounding near half an ulp) and
                         0.49 without, out 0.0060 (fused) and 0.0051 (plain); a_out the bits of as_bn_act_fwd, the plain form on
                         it the fused form's bits, on all 25 geometries and at halo (1, 1)
  as_conv32to1_fwd       out 0.0036, g_up 0.0054, with a border of data 0.0045
  as_conv32to1_bwd       g_a 0.37, g_w 0.011 (accumulating 0.40, on the 1 x 1 map: a sum of two terms), g_bias 8e-4
  ..._dgrad_bnsums       g_a the bits of as_conv32to1_bwd; slabs 0.26 (2 x 3 x 129)
  as_conv4_wgrad         dW 0.013, db 0.0028
  ..._bnapply            g_z 0.65, dW 0.73 and db 0.46 (accumulating, 1 x 1 x 1; at most 0.02 elsewhere)
  ..._bnapply_proj       h 0.073, dW 0.59 and db 0.59 (1 x 1 x 1), g_up through as_tap_gather 0.040, through the thin forward 0.0058
  as_tap_gather          0.16 (with a residual), 0.091 (without)
No defect found in the kernels or their entry points.  One finding about the issue's list of wrong restatements: the own-column
mask of refine_out_kernel taken up to staged voxel 127 changes no word (refine_ends_ref.MUTANTS), so no test can see it.  The
file takes 5.4 s: no case above 0.5 s.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from adaptive_stereo import _native as nat
from adaptive_stereo.hip_ops import Pcl, ConvShape
import refine_ends_ref as rr
from conftest import parity_note

DEV = "cuda:0"
PATTERN = 0x7FF92345        # a quiet NaN that no arithmetic produces
GUARD = 64
S33 = ConvShape(1, 3, 3, 0, 1, 1, 1, 1)
P = nat.ptr


def pcl(geom, halo):
  B, H, W = geom
  return Pcl(B, 1, H, W, 0, halo[0], halo[1])


# ----------------------------------------------------------------------------- buffers
class OutBuf(object):
  """an output with a halo ([B, H + 2 ph, W + 2 pw, C]), every word PATTERN"""

  def __init__(self, g, C=32):
    self.g, self.C = g, C
    self.n = g.B * (g.H + 2 * g.ph) * (g.W + 2 * g.pw) * C
    self.raw = torch.full((GUARD + self.n + GUARD,), PATTERN, dtype=torch.int32, device=DEV)

  def ptr(self):
    return P(self.raw[GUARD:])

  def untouched(self, what):
    torch.cuda.synchronize()
    assert bool((self.raw == PATTERN).all()), "%s: a refused launch wrote %d words" % (what, int((self.raw != PATTERN).sum()))

  def interior(self, what):
    """the interior as fp32 (on the card); asserts guards and halo kept, interior overwritten"""
    torch.cuda.synchronize()
    g, r = self.g, self.raw
    assert bool((r[:GUARD] == PATTERN).all()) and bool((r[-GUARD:] == PATTERN).all()), "%s: wrote outside the tensor" % what
    v = r[GUARD:-GUARD].view(g.B, g.H + 2 * g.ph, g.W + 2 * g.pw, self.C)
    inner = v[:, g.ph:g.ph + g.H, g.pw:g.pw + g.W]
    nhalo = int((v != PATTERN).sum()) - int((inner != PATTERN).sum())
    assert nhalo == 0, "%s: %d halo words were written" % (what, nhalo)
    f = inner.contiguous().view(torch.float32)
    nn = int(torch.isnan(f).sum())
    assert nn == 0, "%s: %d interior elements are NaN (not written, or a guard value was consumed)" % (what, nn)
    return f


class InBuf(object):
  """a channel-last input [B, H, W, C] inside a halo — zeros (a launch that reads it as a value) or PATTERN (a launch that
  must not) — between guard words of PATTERN; `ring`: [B, H + 2, W + 2, C] with data in the one-voxel border instead"""

  def __init__(self, t, g, halo="pattern", ring=None):
    self.raw = torch.full((GUARD + t.numel() // (g.H * g.W) * (g.H + 2 * g.ph) * (g.W + 2 * g.pw) + GUARD,), PATTERN,
                          dtype=torch.int32, device=DEV)
    v = self.raw[GUARD:-GUARD].view(torch.float32).view(g.B, g.H + 2 * g.ph, g.W + 2 * g.pw, t.shape[-1])
    if halo == "zero":
      v.zero_()
    if ring is not None:
      v[:, g.ph - 1:g.ph + g.H + 1, g.pw - 1:g.pw + g.W + 1] = ring.float()
    v[:, g.ph:g.ph + g.H, g.pw:g.pw + g.W] = t.float()

  def ptr(self):
    return P(self.raw[GUARD:])


class Flat(object):
  """numel 4-byte words of output inside a buffer of PATTERN; `init` (fp32) for an accumulating launch"""

  def __init__(self, numel, init=None):
    self.n = numel
    self.raw = torch.full((GUARD + numel + GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    if init is not None:
      self.raw[GUARD:GUARD + numel].view(torch.float32).copy_(init.reshape(-1).to(DEV))

  def ptr(self):
    return P(self.raw[GUARD:])

  def untouched(self, what):
    torch.cuda.synchronize()
    assert bool((self.raw == PATTERN).all()), "%s: a refused launch wrote %d words" % (what, int((self.raw != PATTERN).sum()))

  def guards(self, what):
    torch.cuda.synchronize()
    r = self.raw
    assert bool((r[:GUARD] == PATTERN).all()) and bool((r[-GUARD:] == PATTERN).all()), "%s: wrote outside the destination" % what

  def result(self, what, dtype=torch.float32):
    self.guards(what)
    body = self.raw[GUARD:GUARD + self.n]
    assert not bool((body == PATTERN).any()), "%s: %d words not written" % (what, int((body == PATTERN).sum()))
    v = body.view(dtype)
    assert not bool(torch.isnan(v).any()), "%s: %d NaN" % (what, int(torch.isnan(v).sum()))
    return v


class Worst(object):
  def __init__(self, tag):
    self.tag, self.r, self.extra = tag, {}, {}

  def inside(self, name, got, ref, bound):
    r = rr.ratio(got, ref, bound)
    self.r[name] = max(self.r.get(name, 0.0), r)
    if not r <= 1.0:
      got, ref, bound = got.double().reshape(ref.shape), ref.double(), bound.double().reshape(ref.shape)
      q = ((got - ref).abs() / bound.clamp(min=1e-300)).nan_to_num(float("inf")).reshape(-1)
      i = int(q.argmax())
      raise AssertionError("%s: %s err/bound %.3g at flat index %d (got %r, reference %r, bound %.3e), %d of %d elements over" % (
          self.tag, name, r, i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(bound.reshape(-1)[i]),
          int((q > 1).sum()), q.numel()))

  def ratio(self, name, r):
    self.r[name] = max(self.r.get(name, 0.0), r)
    assert r <= 1.0, "%s: %s err/bound %.3g" % (self.tag, name, r)

  def exact(self, name, got, ref):
    got, ref = got.double().reshape(ref.shape), ref.double()
    assert bool(torch.equal(got, ref)), "%s: %s differs from the exact result in %d of %d elements (largest difference %.3e)" % (
        self.tag, name, int((got != ref).sum()), ref.numel(), float((got - ref).abs().nan_to_num(float("inf")).max()))

  def undecided(self, name, count, numel):
    self.extra["undecided_" + name] = self.extra.get("undecided_" + name, 0) + count
    assert count <= 1e-4 * numel and (numel >= 10 ** 4 or count == 0), "%s: %d of %d elements undecided on %s" % (self.tag, count, numel, name)

  def note(self, **extra):
    parity_note("refine_ends[%s]" % self.tag, **extra, **self.extra, **{"worst_err_over_bound_" + k: v for k, v in self.r.items()})


def _same_bits(a, b, what):
  torch.cuda.synchronize()
  assert bool(torch.equal(a.raw, b.raw)), "%s differ in %d words" % (what, int((a.raw != b.raw).sum()))


def _room(wt, room):
  assert room < 2 ** 24, "%s: an accumulator may reach %.3g quanta: the case is not exact in fp32" % (wt.tag, room)
  wt.note(largest_accumulator_over_2p24=room / 2 ** 24)


# ----------------------------------------------------------------------------- the bit-exact launches
@pytest.mark.parametrize("geom,halo", [((2, 5, 65), (1, 1)), ((1, 1, 1), (1, 1)), ((2, 3, 62), (2, 2)), ((1, 4, 97), (8, 8))],
                         ids=lambda v: "x".join(str(i) for i in v))
def test_pack_in4_is_bit_exact_and_leaves_the_halo(geom, halo):
  B, H, W = geom
  g = pcl(geom, halo)
  gen = torch.Generator().manual_seed(11)
  ch0, img = torch.randn(B, H, W, generator=gen).to(DEV), torch.randn(B, 3, H, W, generator=gen).to(DEV)
  for with0, C in ((True, 3), (False, 3), (True, 1)):
    x4 = OutBuf(g, 4)
    assert nat.load().as_pcl4_numel(g) == x4.n
    im = img[:, :C].contiguous()
    nat.call("as_pack_in4", P(ch0) if with0 else None, P(im), C, x4.ptr(), g, nat.stream())
    assert bool(torch.equal(x4.interior("as_pack_in4"), rr.pack_in4(ch0 if with0 else None, im)))


def test_mirror_taps_ch0_both_layouts():
  w = torch.randn(32, 4, 3, 3, generator=torch.Generator().manual_seed(12)).to(DEV)
  ref_tap, ref_ch = rr.mirror_taps_ch0(w)
  for tap, ch in ((True, True), (True, False), (False, True)):
    bt, bc = Flat(288), Flat(288)
    nat.call("as_mirror_taps_ch0", P(w), 4, bt.ptr() if tap else None, bc.ptr() if ch else None, nat.stream())
    if tap:
      assert bool(torch.equal(bt.result("by_tap").view(9, 32), ref_tap))
    else:
      bt.untouched("by_tap = NULL")
    if ch:
      assert bool(torch.equal(bc.result("by_channel").view(32, 9), ref_ch))
    else:
      bc.untouched("by_channel = NULL")


@pytest.mark.parametrize("n", rr.RELU_BWD_N)
def test_relu_bwd_vector_body_and_scalar_tail(n):
  gen = torch.Generator().manual_seed(13 + n)
  g_out, out = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
  out[::3] = 0.0
  out[1::7] = -0.0
  g_in, g_out, out = Flat(n), g_out.to(DEV), out.to(DEV)
  nat.call("as_relu_bwd", P(g_out), P(out), n, g_in.ptr(), nat.stream())
  got = g_in.result("as_relu_bwd")
  assert bool(torch.equal(got.view(torch.int32), rr.relu_bwd(g_out, out).view(torch.int32))), "g_pre differs (or a -0.0 came out)"


# ----------------------------------------------------------------------------- as_conv4_fwd
def _pack4(w):
  wp = torch.empty(9 * 128, device=DEV)
  nat.call("as_conv4_pack_weights", P(w), 4, P(wp), S33, nat.stream())
  return wp


def _conv4_launch(x4b, g4, g, wp, bias, epilogue, scale=None, shift=None, slope=0.2, moments=False):
  z = OutBuf(g)
  parts = nat.load().as_conv4_stat_parts(g4, g, S33)
  st = [Flat(parts * 32), Flat(parts * 32), Flat(parts)] if moments else [None] * 3
  nat.call("as_conv4_fwd", x4b.ptr(), g4, P(wp), P(bias), z.ptr(), g, S33, epilogue, P(scale), P(shift), slope,
           *[s.ptr() if s else None for s in st], nat.stream())
  for s in st:
    if s:
      s.result("as_conv4_fwd moments")
  return z


CONV4_CASES = [(g, (1, 1)) for g in rr.CONV4_ROWS + rr.CONV4_ONE_TILE] + [(rr.CONV4_HALO2, (2, 2))]
CONV4_IDS = ["%s-halo%d" % (rr.geom_id(g), h[0]) for g, h in CONV4_CASES]


def _conv4_route(geom, halo, g4, g):
  B, H, W = geom
  rows = rr.conv4_rows_route(W, *halo)
  assert rows == (geom in rr.CONV4_ROWS or geom == rr.CONV4_HALO2)
  assert nat.load().as_conv4_stat_parts(g4, g, S33) == rr.conv4_stat_parts(B, H, W, *halo)
  return rows


@pytest.mark.parametrize("geom,halo", CONV4_CASES, ids=CONV4_IDS)
def test_conv4_fwd_against_float64(geom, halo):
  """epilogue 0 without moments (the kernels' mode 2), with moments (equal z bits), epilogue 1; x4 in a zero halo"""
  g4, g = pcl(geom, halo), pcl(geom, (8, 8))
  rows = _conv4_route(geom, halo, g4, g)
  c = rr.case(geom, DEV)
  wt = Worst("conv4 %s halo %d" % (rr.geom_id(geom), halo[0]))
  x4b, wp, st = InBuf(c["x4"], g4, "zero"), _pack4(c["w_in"]), c["st"]
  z = _conv4_launch(x4b, g4, g, wp, c["b_in"], 0)
  f = rr.conv4_forward(c["x4"], c["w_in"], c["b_in"])
  wt.inside("z", z.interior("as_conv4_fwd z"), f["z"], f["e_z"])
  _same_bits(_conv4_launch(x4b, g4, g, wp, c["b_in"], 0, moments=True), z, "z with and without the moments")
  z1 = _conv4_launch(x4b, g4, g, wp, c["b_in"], 1, st["scale"], st["shift"], c["slope"])
  f1 = rr.conv4_forward(c["x4"], c["w_in"], c["b_in"], st["scale"], st["shift"], c["slope"])
  wt.inside("epilogue 1", z1.interior("as_conv4_fwd epilogue 1"), f1["z"], f1["e_z"])
  zn = _conv4_launch(x4b, g4, g, wp, None, 0)
  fn = rr.conv4_forward(c["x4"], c["w_in"], None)
  wt.inside("z without bias", zn.interior("as_conv4_fwd z, bias = NULL"), fn["z"], fn["e_z"])
  wt.note(rows_route=rows, tiles=rr.conv4_tiles(*geom)[0] if rows else 0)


@pytest.mark.parametrize("geom,halo", [c for c in CONV4_CASES if c[0][1] < 100], ids=[i for c, i in zip(CONV4_CASES, CONV4_IDS) if c[0][1] < 100])
def test_conv4_fwd_integer_cases_are_exact(geom, halo):
  g4, g = pcl(geom, halo), pcl(geom, (8, 8))
  _conv4_route(geom, halo, g4, g)
  wt = Worst("conv4 %s halo %d exact" % (rr.geom_id(geom), halo[0]))
  room = 0.0
  for wfam in rr.EXACT_WEIGHTS:
    c = rr.exact_case(geom, wfam, DEV)
    x4b, wp, st, name = InBuf(c["x4"], g4, "zero"), _pack4(c["w_in"]), c["st"], " %s %d" % wfam
    f = rr.conv4_forward(c["x4"], c["w_in"], c["b_in"])
    room = max(room, rr.headroom(f["S"]))
    wt.exact("z" + name, _conv4_launch(x4b, g4, g, wp, c["b_in"], 0, moments=wfam[0] == "dense").interior("z"), f["z"])
    f1 = rr.conv4_forward(c["x4"], c["w_in"], c["b_in"], st["scale"], st["shift"], c["slope"])
    wt.exact("epilogue 1" + name, _conv4_launch(x4b, g4, g, wp, c["b_in"], 1, st["scale"], st["shift"], c["slope"]).interior("z"), f1["z"])
  _room(wt, room)


# ----------------------------------------------------------------------------- as_refine_out_fwd
def _refine_out(xb, skipb, st, slope, g, w, bias, add, relu, a_halo=None):
  """one launch; st None: the plain form.  Returns (a_out or None, out [B, H, W])"""
  a_out = OutBuf(pcl((g.B, g.H, g.W), a_halo or (g.ph, g.pw))) if st is not None else None
  out = Flat(g.B * g.H * g.W)
  nat.call("as_refine_out_fwd", xb.ptr(), skipb.ptr() if skipb else None, P(st["scale"]) if st else None, P(st["shift"]) if st else None,
           slope, a_out.ptr() if a_out else None, g, P(w), P(bias), P(add), relu, out.ptr(), nat.stream())
  return a_out, out.result("as_refine_out_fwd out").view(g.B, g.H, g.W)


def _refine_out_forms(geom, halo, c, wt, exact=False, name=""):
  g = pcl(geom, halo)
  assert nat.load().as_refine_out_ok(g) == 1 and rr.refine_out_ok(1, 0, halo[0], halo[1], geom[2])
  st, sl, w = c["st"], c["slope"], c["w_out"]
  zb, sb, ab = InBuf(c["z"], g), InBuf(c["skip"], g), InBuf(c["a"], g)
  judge = (lambda n, got, ref, e: wt.exact(n + name, got, ref)) if exact else wt.inside
  room = 0.0
  # the activation fused, with and without the skip connection
  for skip, relu, bias, add in ((True, 1, c["b_out"], c["up"]), (False, 0, None, None)) + (((True, 0, None, c["up"]),) if not exact else ()):
    a_out, out = _refine_out(zb, sb if skip else None, st, sl, g, w, bias, add, relu)
    tag = "skip" if skip else "no skip"
    a32 = a_out.interior("as_refine_out_fwd a_out (%s)" % tag)
    a_ref, e_a = rr.act_chain(c["z"], c["skip"] if skip else None, st["scale"], st["shift"], sl)
    judge("a_out " + tag, a32, a_ref, e_a)
    o = rr.out_layer(a32, w, bias, add, relu)
    room = max(room, rr.headroom(o["S"]))
    judge("out " + tag, out, o["out"], o["e_out"])
    # the two launches it replaces: the by-product bit for bit; the plain form on it: the fused form's bits
    a_two = OutBuf(g)
    nat.call("as_bn_act_fwd", zb.ptr(), P(st["scale"]), P(st["shift"]), sl, sb.ptr() if skip else None, a_two.ptr(), g, nat.stream())
    _same_bits(a_two, a_out, "a_out of as_refine_out_fwd and of as_bn_act_fwd (%s)" % tag)
    _, out_p = _refine_out(a_two, None, None, sl, g, w, bias, add, relu)
    assert bool(torch.equal(out_p, out)), "the plain form on the fused form's a_out gives other bits (%s)" % tag
  # the plain form on an input of its own (12-row strips)
  for relu, bias, add in ((1, c["b_out"], None), (0, None, c["up"])):
    _, out = _refine_out(ab, None, None, sl, g, w, bias, add, relu)
    o = rr.out_layer(c["a"], w, bias, add, relu)
    room = max(room, rr.headroom(o["S"]))
    judge("plain out", out, o["out"], o["e_out"])
  return room


@pytest.mark.parametrize("geom", rr.REFINE_OUT, ids=rr.geom_id)
def test_refine_out_against_float64(geom):
  wt = Worst("refine_out %s" % rr.geom_id(geom))
  _refine_out_forms(geom, (8, 8), rr.case(geom, DEV), wt)
  wt.note(workgroups_act=rr.ro_grid(*geom, True)[2], workgroups_plain=rr.ro_grid(*geom, False)[2])


@pytest.mark.parametrize("geom", rr.REFINE_OUT, ids=rr.geom_id)
def test_refine_out_integer_cases_are_exact(geom):
  wt = Worst("refine_out %s exact" % rr.geom_id(geom))
  _room(wt, max(_refine_out_forms(geom, (8, 8), rr.exact_case(geom, wfam, DEV), wt, True, " %s %d" % wfam) for wfam in rr.EXACT_WEIGHTS))


def test_refine_out_at_its_floor_halo_1_1_width_126():
  """accepted: the staged row of the last image's last row ends exactly at the buffer's end (the guard words behind it are NaN)"""
  geom = rr.REFINE_OUT_HALO1
  wt = Worst("refine_out %s halo 1" % rr.geom_id(geom))
  _refine_out_forms(geom, (1, 1), rr.case(geom, DEV), wt)
  _room(wt, _refine_out_forms(geom, (1, 1), rr.exact_case(geom, ("dense", 0), DEV), wt, True, " dense"))


REFUSALS = ["halo (1, 1) W 125", "D 2", "pd 1", "a_out is x", "a_out is skip", "scale without a_out", "skip without scale", "slope 0",
            "slope 1"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refine_out_refusals_write_nothing(what):
  lib = nat.load()
  B, H, W = 2, 5, 126
  g = Pcl(B, 1, H, W, 0, 8, 8)
  if what == "halo (1, 1) W 125":
    g = Pcl(B, 1, H, 125, 0, 1, 1)
  elif what == "D 2":
    g = Pcl(B, 2, H, W, 0, 8, 8)
  elif what == "pd 1":
    g = Pcl(B, 1, H, W, 1, 8, 8)
  geometry = what in REFUSALS[:3]
  assert lib.as_refine_out_ok(g) == (0 if geometry else 1)
  n = g.numel()
  x, skip = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
  a_out, out = Flat(n), Flat(B * 2 * H * W)
  vec, w = torch.ones(32, device=DEV), torch.zeros(288, device=DEV)
  args = dict(x=P(x), skip=P(skip), scale=P(vec), shift=P(vec), slope=0.2, a_out=a_out.ptr())
  if what == "a_out is x":
    args["a_out"] = P(x)
  elif what == "a_out is skip":
    args["a_out"] = P(skip)
  elif what == "scale without a_out":
    args["a_out"] = None
  elif what == "skip without scale":
    args.update(scale=None, shift=None, a_out=None)
  elif what == "slope 0":
    args["slope"] = 0.0
  elif what == "slope 1":
    args["slope"] = 1.0
  rc = lib.as_refine_out_fwd(args["x"], args["skip"], args["scale"], args["shift"], args["slope"], args["a_out"], g, P(w), None, None, 1,
                             out.ptr(), nat.stream())
  assert rc == -1, "as_refine_out_fwd accepted %s (status %d)" % (what, rc)
  if geometry:
    assert "not supported" in lib.as_last_error().decode()
  a_out.untouched(what)
  out.untouched(what)
  assert float(x.abs().max()) == 0.0 and float(skip.abs().max()) == 0.0


# ----------------------------------------------------------------------------- as_conv32to1_fwd, thin 2-D
def _thin_fwd(ab, g, w, bias, add, relu):
  out = Flat(g.B * g.H * g.W)
  nat.call("as_conv32to1_fwd", ab.ptr(), g, S33, P(w), P(bias), P(add), relu, out.ptr(), nat.stream())
  return out.result("as_conv32to1_fwd out").view(g.B, g.H, g.W)


def _mirrored_by_channel(w_in):
  bc = Flat(288)
  nat.call("as_mirror_taps_ch0", P(w_in), 4, None, bc.ptr(), nat.stream())
  return bc.result("by_channel").view(32, 9).clone()


THIN_FWD_CASES = [(g, h) for g in rr.THIN_FWD for h in ((8, 8), (1, 1))]


@pytest.mark.parametrize("geom,halo", THIN_FWD_CASES, ids=["%s-halo%d" % (rr.geom_id(g), h[0]) for g, h in THIN_FWD_CASES])
def test_thin_forward_against_float64(geom, halo):
  """the output layer (bias, add_src, ReLU), the g_up use (w_ch0 from as_mirror_taps_ch0, add_src = g_pre, no ReLU), and once
  with data in the one-voxel border the kernel reads as values; the exact family on the first two"""
  B, H, W = geom
  g = pcl(geom, halo)
  assert nat.load().as_conv32to1_bnsums_ok(g, S33) == 1            # (the thin route's own test)
  c = rr.case(geom, DEV)
  wt = Worst("thin fwd %s halo %d" % (rr.geom_id(geom), halo[0]))
  ab = InBuf(c["a"], g, "zero")
  o = rr.out_layer(c["a"], c["w_out"], c["b_out"], c["up"], 1)
  wt.inside("out", _thin_fwd(ab, g, c["w_out"], c["b_out"], c["up"], 1), o["out"], o["e_out"])
  w_ch0 = _mirrored_by_channel(c["w_in"])
  assert bool(torch.equal(w_ch0, rr.mirror_taps_ch0(c["w_in"])[1]))
  g_pre = rr.relu_bwd(c["g_out"], c["out"])
  gzb = InBuf(c["g_a"], g, "zero")
  u = rr.out_layer(c["g_a"], w_ch0, None, g_pre, 0)
  wt.inside("g_up", _thin_fwd(gzb, g, w_ch0, None, g_pre, 0), u["out"], u["e_out"])
  ring = torch.randn(B, H + 2, W + 2, 32, generator=torch.Generator().manual_seed(H * 1000 + W)).to(DEV)
  ring[:, 1:H + 1, 1:W + 1] = c["a"]
  r = rr.out_layer(c["a"], c["w_out"], None, None, 0, ring=ring)
  wt.inside("out with a border of data", _thin_fwd(InBuf(c["a"], g, "zero", ring=ring), g, c["w_out"], None, None, 0), r["out"], r["e_out"])
  room = 0.0
  for wfam in rr.EXACT_WEIGHTS:
    e = rr.exact_case(geom, wfam, DEV)
    o = rr.out_layer(e["a"], e["w_out"], e["b_out"], e["up"], 1)
    room = max(room, rr.headroom(o["S"]))
    wt.exact("out %s %d" % wfam, _thin_fwd(InBuf(e["a"], g, "zero"), g, e["w_out"], e["b_out"], e["up"], 1), o["out"])
  _room(wt, room)


# ----------------------------------------------------------------------------- as_conv32to1_bwd, as_conv32to1_dgrad_bnsums
def _thin_bwd(g_pre, ab, g, w, want_g_a, g_w0=None, g_b0=None):
  lib = nat.load()
  g_a = OutBuf(g) if want_g_a else None
  acc = 1 if g_w0 is not None else 0
  g_w, g_b, ws = Flat(288, g_w0), Flat(1, g_b0), Flat(lib.as_conv32to1_bwd_workspace(g, S33))
  nat.call("as_conv32to1_bwd", P(g_pre), ab.ptr(), g, S33, P(w), g_a.ptr() if g_a else None, g_w.ptr(), g_b.ptr(), acc, ws.ptr(), nat.stream())
  ws.guards("as_conv32to1_bwd workspace")
  return g_a, g_w.result("g_w").view(32, 9), g_b.result("g_bias")


def _bnsums(g_pre, zb, g, w, st, slope):
  parts = nat.load().as_conv32to1_bnsums_parts(g)
  g_a, slabs = OutBuf(g), Flat(parts * 128)
  nat.call("as_conv32to1_dgrad_bnsums", P(g_pre), g, S33, P(w), g_a.ptr(), zb.ptr(), P(st["scale"]), P(st["shift"]), P(st["mean"]), slope,
           slabs.ptr(), nat.stream())
  return g_a, slabs.result("bnsums slabs", torch.float64).view(parts, 64), parts


@pytest.mark.parametrize("geom", rr.THIN_BWD, ids=rr.geom_id)
def test_thin_backward_against_float64(geom):
  """g_a given, accumulate 0; g_a NULL, accumulate 1 on a non-zero g_w; the exact family on all but the cap case"""
  B, H, W = geom
  g = pcl(geom, (8, 8))
  assert nat.load().as_conv32to1_bnsums_ok(g, S33) == 1
  c = rr.case(geom, DEV)
  wt = Worst("thin bwd %s" % rr.geom_id(geom))
  g_pre, ab = rr.relu_bwd(c["g_out"], c["out"]).contiguous(), InBuf(c["a"], g, "zero")
  g_a, g_w, g_b = _thin_bwd(g_pre, ab, g, c["w_out"], True)
  d = rr.data_gradient(g_pre, c["w_out"])
  wt.inside("g_a", g_a.interior("as_conv32to1_bwd g_a"), d["g_a"], d["e_g_a"])
  wg = rr.weight_gradient(c["a"], g_pre)
  wt.inside("g_w", g_w, wg["g_w"], wg["e_g_w"])
  wt.inside("g_bias", g_b, wg["g_b"], wg["e_g_b"])
  _, g_w, g_b = _thin_bwd(g_pre, ab, g, c["w_out"], False, c["g_w0"], c["g_b0"])
  wg = rr.weight_gradient(c["a"], g_pre, c["g_w0"], c["g_b0"])
  wt.inside("g_w accumulate", g_w, wg["g_w"], wg["e_g_w"])
  wt.inside("g_bias accumulate", g_b, wg["g_b"], wg["e_g_b"])
  wt.note(chunks=rr.chunks(B, H, W)[1], dgrad_workgroups=rr.dgrad_grid(B, H, W), wgrad_workgroups=rr.wgrad_grid(B, H, W))
  if rr.chunks(B, H, W)[1] > 1024:
    return
  room = 0.0
  for wfam in rr.EXACT_WEIGHTS:
    e = rr.exact_case(geom, wfam, DEV)
    name = " %s %d" % wfam
    g_a, g_w, g_b = _thin_bwd(e["g_out"], InBuf(e["a"], g, "zero"), g, e["w_out"], True, e["g_w0"], e["g_b0"])
    wt.exact("g_a" + name, g_a.interior("g_a"), rr.thin_dgrad_sum(e["g_out"], e["w_out"])[0])
    wg = rr.weight_gradient(e["a"], e["g_out"], e["g_w0"], e["g_b0"])
    wt.exact("g_w accumulate" + name, g_w, wg["g_w"])
    wt.exact("g_bias accumulate" + name, g_b, wg["g_b"])
    room = max(room, rr.headroom(rr.thin_wgrad_sum(e["a"].abs(), e["g_out"].abs())[0] + e["g_w0"].abs()))
  _room(wt, room)


def test_thin_data_gradient_beyond_its_grid_cap():
  """16388 chunks on 16384 workgroups: the chunk loop of the data gradient strides (38 MB of g_a with its halo)"""
  geom = rr.THIN_BWD_DGRAD_CAP
  B, H, W = geom
  assert rr.chunks(B, H, W)[1] > rr.DGRAD_CAP
  g = pcl(geom, (8, 8))
  gen = torch.Generator().manual_seed(14)
  g_pre = rr.sentinels(torch.randn(B, H, W, generator=gen)).to(DEV)
  w = (torch.randn(32, 9, generator=gen) * 0.2).to(DEV)
  g_a = OutBuf(g)
  ws = Flat(nat.load().as_conv32to1_bwd_workspace(g, S33))
  a = torch.zeros(1, device=DEV)                                 # (not read: no weight gradient is asked for)
  nat.call("as_conv32to1_bwd", P(g_pre), P(a), g, S33, P(w), g_a.ptr(), None, None, 0, ws.ptr(), nat.stream())
  ws.untouched("as_conv32to1_bwd workspace without a weight gradient")
  wt = Worst("thin bwd %s" % rr.geom_id(geom))
  d = rr.data_gradient(g_pre, w)
  wt.inside("g_a", g_a.interior("as_conv32to1_bwd g_a"), d["g_a"], d["e_g_a"])
  wt.note(chunks=rr.chunks(B, H, W)[1])


@pytest.mark.parametrize("geom", rr.BNSUMS, ids=rr.geom_id)
def test_dgrad_bnsums_against_float64(geom):
  """g_a: the bits of as_conv32to1_bwd; the fp64 slabs per partial over the chunks ch = blk (mod grid)"""
  B, H, W = geom
  g = pcl(geom, (8, 8))
  lib = nat.load()
  assert lib.as_conv32to1_bnsums_ok(g, S33) == 1 and lib.as_conv32to1_bnsums_parts(g) == rr.bnsums_parts(B, H, W)
  wt = Worst("bnsums %s" % rr.geom_id(geom))
  c = rr.case(geom, DEV)
  st, sl = c["st"], c["slope"]
  g_pre = rr.relu_bwd(c["g_out"], c["out"]).contiguous()
  g_a, slabs, parts = _bnsums(g_pre, InBuf(c["z"], g), g, c["w_out"], st, sl)
  g_a2, _, _ = _thin_bwd(g_pre, InBuf(c["a"], g, "zero"), g, c["w_out"], True)
  _same_bits(g_a, g_a2, "g_a of as_conv32to1_dgrad_bnsums and of as_conv32to1_bwd")
  s = rr.bn_sums(g_a.interior("g_a"), c["z"], st["scale"], st["shift"], st["mean"], sl, parts)
  wt.undecided("y", s["undecided"], c["z"].numel())
  wt.inside("slabs", slabs, s["sums"], s["e_sums"])
  e = rr.exact_case(geom, ("dense", 0), DEV)
  g_a, slabs, parts = _bnsums(e["g_out"], InBuf(e["z"], g), g, e["w_out"], e["st"], e["slope"])
  s = rr.bn_sums(g_a.interior("g_a"), e["z"], e["st"]["scale"], e["st"]["shift"], e["st"]["mean"], e["slope"], parts)
  wt.exact("slabs dense", slabs, s["sums"])
  wt.note(chunks=rr.chunks(B, H, W)[1], partials=parts)


# ----------------------------------------------------------------------------- the conv4 weight gradients, as_tap_gather
class Wgrad4(object):
  def __init__(self, geom, c, halo4=(1, 1)):
    self.lib, self.geom, self.c = nat.load(), geom, c
    self.g4, self.g = pcl(geom, halo4), pcl(geom, (8, 8))
    assert self.lib.as_conv4_wgrad_bnapply_ok(self.g4, self.g, S33) == 1
    self.x4b = InBuf(c["x4"], self.g4, "zero")
    self.gab, self.zb = InBuf(c["g_a"], self.g), InBuf(c["z"], self.g)

  def _outs(self, acc):
    c = self.c
    return Flat(32 * 36, c["dW0"] if acc else None), Flat(32, c["db0"] if acc else None), Flat(self.lib.as_conv4_wgrad_workspace(self.g, S33))

  def _done(self, dW, db, ws, what):
    ws.guards(what + " workspace")
    return dW.result(what + " dW").view(32, 4, 3, 3), db.result(what + " db")

  def plain(self, acc):
    dW, db, ws = self._outs(acc)
    nat.call("as_conv4_wgrad", self.x4b.ptr(), self.g4, self.gab.ptr(), self.g, S33, 4, dW.ptr(), db.ptr(), acc, ws.ptr(), nat.stream())
    return self._done(dW, db, ws, "as_conv4_wgrad")

  def _bn(self, coef):
    st = self.c["st"]
    return (4, P(st["scale"]), P(st["shift"]), P(st["mean"]), P(coef), self.c["slope"])

  def bnapply(self, coef, acc):
    dW, db, ws = self._outs(acc)
    gz = OutBuf(self.g)
    nat.call("as_conv4_wgrad_bnapply", self.x4b.ptr(), self.g4, self.gab.ptr(), self.zb.ptr(), self.g, S33, *self._bn(coef), gz.ptr(),
             dW.ptr(), db.ptr(), acc, ws.ptr(), nat.stream())
    return (gz.interior("as_conv4_wgrad_bnapply g_z"),) + self._done(dW, db, ws, "as_conv4_wgrad_bnapply")

  def proj(self, coef, w_proj, acc):
    B, H, W = self.geom
    dW, db, ws = self._outs(acc)
    h = Flat(B * 9 * H * W)
    nat.call("as_conv4_wgrad_bnapply_proj", self.x4b.ptr(), self.g4, self.gab.ptr(), self.zb.ptr(), self.g, S33, *self._bn(coef),
             P(w_proj), h.ptr(), dW.ptr(), db.ptr(), acc, ws.ptr(), nat.stream())
    return (h.result("as_conv4_wgrad_bnapply_proj h").view(B, 9, H, W),) + self._done(dW, db, ws, "as_conv4_wgrad_bnapply_proj")


def _gather(h, res, geom):
  B, H, W = geom
  out = Flat(B * H * W)
  nat.call("as_tap_gather", P(h), P(res), out.ptr(), B, H, W, nat.stream())
  return out.result("as_tap_gather").view(B, H, W)


def _by_tap(w_in):
  bt = Flat(288)
  nat.call("as_mirror_taps_ch0", P(w_in), 4, bt.ptr(), None, nat.stream())
  return bt.result("by_tap").view(9, 32).clone()


WGRAD4_CASES = [(g, (1, 1)) for g in rr.CONV4_WGRAD] + [(rr.CONV4_WGRAD_HALO2, (2, 2))]


@pytest.mark.parametrize("geom,halo4", WGRAD4_CASES, ids=["%s-halo%d" % (rr.geom_id(g), h[0]) for g, h in WGRAD4_CASES])
def test_conv4_weight_gradients_against_float64(geom, halo4):
  """as_conv4_wgrad (accumulate 0), as_conv4_wgrad_bnapply (accumulate 1), as_conv4_wgrad_bnapply_proj (accumulate 0) with the
  coefficients of bn_ref.bn_bwd64 on the case's own data, and both routes to g_up against the same float64 g_up"""
  B, H, W = geom
  c = rr.case(geom, DEV)
  wt = Worst("conv4 wgrad %s halo %d" % (rr.geom_id(geom), halo4[0]))
  L = Wgrad4(geom, c, halo4)
  st, sl, n = c["st"], c["slope"], c["z"].numel()
  dW, db = L.plain(0)
  w4 = rr.conv4_weight_gradient(c["x4"], c["g_a"])
  wt.inside("dW", dW, w4["dW"], w4["e_dW"])
  wt.inside("db", db, w4["db"], w4["e_db"])
  coef = rr.bn_coef(c["g_a"], c["z"], st, c["gamma"], sl).float().to(DEV)
  ref = rr.gz_chain(c["g_a"], c["z"], st["scale"], st["shift"], st["mean"], coef, sl)
  gz32, dW, db = L.bnapply(coef, 1)
  r, und = rr.judge_gz(gz32, ref)
  wt.undecided("y", und, n)
  wt.ratio("g_z", r)
  w4 = rr.conv4_weight_gradient(c["x4"], gz32, c["dW0"], c["db0"])
  wt.inside("bnapply dW accumulate", dW, w4["dW"], w4["e_dW"])
  wt.inside("bnapply db accumulate", db, w4["db"], w4["e_db"])
  w_proj = _by_tap(c["w_in"])
  h32, dW, db = L.proj(coef, w_proj, 0)
  p = rr.proj_planes(ref, c["w_in"])
  wt.ratio("h", rr.judge_h(h32, p))
  both = rr.gz_both(ref)
  w4 = rr.conv4_weight_gradient(c["x4"], ref["g_z"], None, None, rr.gz_bound(ref), both)
  wt.inside("proj dW", dW, w4["dW"], w4["e_dW"])
  wt.inside("proj db", db, w4["db"], w4["e_db"])
  # the two routes to the disparity channel's data gradient, against the same float64 g_up
  g_pre = rr.relu_bwd(c["g_out"], c["out"]).contiguous()
  w_ch0 = _mirrored_by_channel(c["w_in"])
  g_up = rr.g_up64(ref["g_z"], c["w_in"], g_pre)
  carried = rr.conv_out_sum(rr.gz_bound(ref) + both, w_ch0.abs())
  a = rr.out_layer(gz32, w_ch0, None, g_pre, 0)
  wt.inside("g_up by the thin forward", _thin_fwd(InBuf(gz32, L.g, "zero"), L.g, w_ch0, None, g_pre, 0), g_up, a["e_out"] + carried)
  t = rr.tap_gather(h32, g_pre)
  wt.inside("g_up by projections", _gather(h32, g_pre, geom), g_up, t["e_out"] + rr.tap_gather_sum(p["e_h"] + rr.proj_sum(both, c["w_in"].abs())))
  wt.note(chunks=rr.chunks(B, H, W)[1], workgroups=rr.wgrad_grid(B, H, W))
  if rr.chunks(B, H, W)[1] > 1024:
    return
  room = 0.0
  for wfam in rr.EXACT_WEIGHTS:
    e = rr.exact_case(geom, wfam, DEV)
    E, name = Wgrad4(geom, e, halo4), " %s %d" % wfam
    ref = rr.gz_chain(e["g_a"], e["z"], e["st"]["scale"], e["st"]["shift"], e["st"]["mean"], e["coef"], e["slope"])
    dWr, dbr = rr.conv4_wgrad_sum(e["x4"], ref["g_z"])
    gz32, dW, db = E.bnapply(e["coef"], 1)
    wt.exact("g_z" + name, gz32, ref["g_z"])
    wt.exact("bnapply dW accumulate" + name, dW, dWr + e["dW0"].double())
    wt.exact("bnapply db accumulate" + name, db, dbr + e["db0"].double())
    h32, dW, db = E.proj(e["coef"], _by_tap(e["w_in"]), 0)
    wt.exact("h" + name, h32, rr.proj_sum(ref["g_z"], e["w_in"]))
    wt.exact("proj dW" + name, dW, dWr)
    wt.exact("proj db" + name, db, dbr)
    wt.exact("g_up" + name, _gather(h32, e["g_out"], geom), rr.g_up64(ref["g_z"], e["w_in"], e["g_out"]))
    room = max(room, rr.headroom(rr.conv4_wgrad_sum(e["x4"].abs(), ref["g_z"].abs())[0] + e["dW0"].abs(), rr.proj_sum(ref["g_z"].abs(), e["w_in"].abs())))
  _room(wt, room)


@pytest.mark.parametrize("geom", rr.TAP_GATHER, ids=rr.geom_id)
def test_tap_gather_against_float64(geom):
  B, H, W = geom
  gen = torch.Generator().manual_seed(15 + 131 * H + W)
  h = rr.sentinels(torch.randn(B, H, W, 9, generator=gen)).permute(0, 3, 1, 2).contiguous()
  h, res = h.to(DEV), rr.sentinels(torch.randn(B, H, W, generator=gen)).to(DEV)
  hi, ri = torch.randint(-4, 5, (B, 9, H, W), generator=gen).float().to(DEV), torch.randint(-4, 5, (B, H, W), generator=gen).float().to(DEV)
  wt = Worst("tap gather %s" % rr.geom_id(geom))
  for r, ir in ((res, ri), (None, None)):
    t = rr.tap_gather(h, r)
    wt.inside("out" if r is not None else "out without residual", _gather(h, r, geom), t["out"], t["e_out"])
    wt.exact("integers", _gather(hi, ir, geom), rr.tap_gather_sum(hi, ir))
  wt.note()
