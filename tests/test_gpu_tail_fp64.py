"""The two ends of the cost-aggregation chain through the C ABI, ONE LAUNCH AT A TIME, against the float64 restatements and the
derived bounds of tests/tail_ref.py (held to torch on the CPU, and shown to discriminate, by tests/test_tail_ref_cpu.py):
as_cost_volume_fwd / _bwd, the fused tail as_agg_tail_fwd (32 -> 1 convolution, soft-argmax, arg-max, FCS), its one-launch
backward as_agg_tail_bwd, and the first-generation launches as_conv3d_out_fwd / _bwd and as_softargmax_fwd / _bwd, at the
smallest shapes that reach each kernel and each side of each threshold.  The dispatch counts tiles and units, not voxels: many
small images reach the 32-position forward and the 26-column backward with a few MB.

Every case first asserts its route through the read-only queries as_agg_tail_fwd_positions / as_agg_tail_bwd_columns (and
as_agg_tail_ok / as_agg_tail_bwd_ok): the routes give equal logits by design, so nothing else could tell which kernel ran.

Every output sits between guard words of one NaN bit pattern and starts as that pattern: every interior element must be
overwritten, the guards must keep it, the halo of g_a and vol must keep what it held, and the halo of a_out — zero before — must
be exactly zero afterwards (the forward's unconditional by-product stores write the zeros they loaded there).  The activation
the backward reads and the volume gradient of the cost volume's adjoint carry the pattern in their halo: it must not be consumed.

Random family (sentinels of +-1e4 on the first and last plane, row and column; w and bias at gains 1, 50 and 300): logits against
float64; pred and FCS against float64 on the kernel's OWN logits; arg-max equal to the first maximum of the kernel's own logits
everywhere and to the reference's wherever the reference decides (top-2 gap > 2 max_d e_logit; at most 1 % undecided).  Exact
families (single-tap weights, designed ties and extremes, integer gradients, two-impulse activations) are bit-exact.  No element
is left out of a comparison.  The worst err / bound of every output goes to conftest.parity_note (tail[...]).

K_EXP = 2 is in force (tail_ref.K_EXP: 1 ulp for a library expf, the same again as margin; not fitted).
Worst err / bound seen on an MI355X, per entry point:
  as_agg_tail_fwd      logits 0.0071 (affine input 0.0075), a_out 0.25, pred 0.81 on 16 positions (511 x 3 x 1 x 32) and 0.80 on 32
                       (512 x 3 x 1 x 32; affine 0.81), FCS 0.47 (171 x 5 x 2 x 40); at D = 2, where pred = e / (1 + e) isolates one
                       exponential, pred 0.44 (affine 0.67): the exponential term stays under 1 with K_EXP = 2
  as_conv3d_out_fwd + as_softargmax_fwd     logits 0.0095, pred 0.80 (0.79 at D = 2), FCS 0.38
  as_agg_tail_bwd      g_a 0.31, g_w 0.48 and g_bias 0.08 (both on 1 x 3 x 1 x 1, sums of three terms; g_w <= 0.1 from 2 x 2 x 3 x 13
                       up, 1e-3 and below on the shapes with two units per workgroup)
  as_softargmax_bwd + as_conv3d_out_bwd     g_logits 0.99 (the one rounding of the final add against U |g_logits|: as tight as a
                       bound of one rounding gets, and never above it), g_a 0.27, g_w 0.48, g_bias 0.08
  as_cost_volume_fwd   bit-exact;  as_cost_volume_bwd   gL 0.49, gR 0.50
Every single-tap, designed, integer-gradient and two-impulse case was bit-exact, every arg-max was the first maximum of the
kernel's own logits, at most 0.98 % of a case's pixels were undecided (one pixel of 102).  No defect found in the kernels.
The file takes 9 s.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from adaptive_stereo import _native as nat
from adaptive_stereo import hip_ops as ops
from adaptive_stereo.hip_ops import Pcl
import tail_ref as tr
from conftest import parity_note

DEV = "cuda:0"
PATTERN = 0x7FF92345        # a quiet NaN that no arithmetic produces
GUARD = 64
SLOPE = 0.2
SMALL = 20000               # voxels up to which a geometry runs every combination


# ----------------------------------------------------------------------------- buffers
def _pattern(n):
  return torch.full((n,), PATTERN, dtype=torch.int32)


class PclBuf(object):
  """a PCL tensor [B, D + 2, H + 2, W + 2, 32] between guards of PATTERN.  interior: [B, D, H, W, 32] values, or None (PATTERN: an
  output); halo: "zero" or "pattern" """

  def __init__(self, g, interior=None, halo="zero"):
    self.g = g
    body = _pattern(g.numel()).view(torch.float32).view(g.B, g.D + 2 * g.pd, g.H + 2 * g.ph, g.W + 2 * g.pw, 32)
    if halo == "zero":
      body.zero_()
    inner = body[:, g.pd:g.pd + g.D, g.ph:g.ph + g.H, g.pw:g.pw + g.W]
    if interior is None:
      inner.copy_(_pattern(1).view(torch.float32).expand_as(inner))
    else:
      inner.copy_(interior.float())
    raw = torch.cat([_pattern(GUARD), body.reshape(-1).view(torch.int32), _pattern(GUARD)])
    self.halo_word = 0 if halo == "zero" else PATTERN
    self.raw = raw.to(DEV)
    self.body = self.raw[GUARD:GUARD + g.numel()].view(torch.float32)

  def ptr(self):
    return nat.ptr(self.body)

  def interior(self, what):
    """guards kept, the halo as it was (bit for bit), every interior element written; returns the interior [B, D, H, W, 32]"""
    torch.cuda.synchronize()
    g = self.g
    r = self.raw.cpu()
    assert bool((r[:GUARD] == PATTERN).all()) and bool((r[-GUARD:] == PATTERN).all()), "%s: wrote outside the tensor" % what
    v = r[GUARD:-GUARD].view(g.B, g.D + 2 * g.pd, g.H + 2 * g.ph, g.W + 2 * g.pw, 32)
    inner = v[:, g.pd:g.pd + g.D, g.ph:g.ph + g.H, g.pw:g.pw + g.W].contiguous()
    halo = v.clone()
    halo[:, g.pd:g.pd + g.D, g.ph:g.ph + g.H, g.pw:g.pw + g.W] = self.halo_word
    assert bool((halo == self.halo_word).all()), "%s: %d halo words changed" % (what, int((halo != self.halo_word).sum()))
    f = inner.view(torch.float32)
    assert not bool(torch.isnan(f).any()), "%s: %d interior elements are NaN (not written, or a guard value was consumed)" % (
        what, int(torch.isnan(f).sum()))
    return f


class Flat(object):
  """numel 4-byte words inside a buffer of PATTERN: an output (init None), an accumulating output or an input (init given)"""

  def __init__(self, numel, init=None, dtype=torch.float32):
    self.dtype = dtype
    self.raw = torch.full((GUARD + numel + GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    self.body = self.raw[GUARD:GUARD + numel].view(dtype)
    if init is not None:
      self.body.copy_(init.reshape(-1).to(DEV))

  def ptr(self):
    return nat.ptr(self.body)

  def guards_kept(self, what):
    torch.cuda.synchronize()
    r = self.raw.cpu()
    assert bool((r[:GUARD] == PATTERN).all()) and bool((r[-GUARD:] == PATTERN).all()), "%s: wrote outside the destination" % what
    return r[GUARD:-GUARD]

  def result(self, what):
    v = self.guards_kept(what)
    assert not bool((v == PATTERN).any()), "%s: %d elements not written" % (what, int((v == PATTERN).sum()))
    v = v.view(self.dtype)
    if self.dtype == torch.float32:
      assert not bool(torch.isnan(v).any()), "%s: %d elements are NaN (a guard value was consumed)" % (what, int(torch.isnan(v).sum()))
    return v


class Worst(object):
  def __init__(self, tag):
    self.tag, self.r = tag, {}

  def inside(self, name, got, ref, bound):
    got, ref, bound = got.double().reshape(ref.shape), ref.double(), bound.double().reshape(ref.shape)
    r = tr.ratio(got, ref, bound)
    self.r[name] = max(self.r.get(name, 0.0), r)
    print("  tail[%s] %s err/bound %.4f" % (self.tag, name, r))
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
    parity_note("tail[%s]" % self.tag, **extra, **{"worst_err_over_bound_" + k: round(v, 4) for k, v in self.r.items()})


def _dev(t):
  return None if t is None else t.float().contiguous().to(DEV)


# ----------------------------------------------------------------------------- the fused forward
class TailOut(object):
  def __init__(self, g, want_argmax=True, want_fcs=True):
    n = g.B * g.H * g.W
    self.g = g
    self.logits, self.pred = Flat(n * g.D), Flat(n)
    self.am = Flat(n, dtype=torch.int32) if want_argmax else None
    self.fcs = Flat(n) if want_fcs else None

  def read(self, what):
    g = self.g
    out = dict(logits=self.logits.result(what + " logits").view(g.B, g.D, g.H, g.W),
               pred=self.pred.result(what + " pred").view(g.B, g.H, g.W))
    if self.am is not None:
      out["argmax"] = self.am.result(what + " argmax").view(g.B, g.H, g.W).long()
    if self.fcs is not None:
      out["fcs"] = self.fcs.result(what + " fcs").view(g.B, g.H, g.W)
    return out


def _tail(x_buf, g, w, b, scale=None, shift=None, in_bn=None, a_out=None, want_argmax=True, want_fcs=True):
  out = TailOut(g, want_argmax, want_fcs)
  nat.call("as_agg_tail_fwd", x_buf.ptr(), g, nat.ptr(scale), nat.ptr(shift), in_bn.block if in_bn is not None else None,
           a_out.ptr() if a_out is not None else None, nat.ptr(w), nat.ptr(b), SLOPE, out.logits.ptr(), out.pred.ptr(),
           out.am.ptr() if out.am is not None else None, out.fcs.ptr() if out.fcs is not None else None, nat.stream())
  return out


def _first_generation(x_buf, g, w, b):
  out = TailOut(g)
  nat.call("as_conv3d_out_fwd", x_buf.ptr(), g, nat.ptr(w), nat.ptr(b), out.logits.ptr(), nat.stream())
  nat.call("as_softargmax_fwd", out.logits.ptr(), g.B, g.D, g.H, g.W, out.pred.ptr(), out.am.ptr(), out.fcs.ptr(), nat.stream())
  return out


def _judge_soft(wt, pre, got, D):
  """pred, fcs and arg-max of one launch against float64 on ITS OWN logits"""
  s = tr.soft_stage(got["logits"])
  wt.inside(pre + "pred", got["pred"], s["pred"], s["e_pred"])
  if "fcs" in got:
    if D > 2:
      wt.inside(pre + "fcs", got["fcs"], s["fcs"], s["e_fcs"])
    else:
      assert float(got["fcs"].abs().max()) == 0.0, "%s: fcs must be 0 for D <= 2" % wt.tag
  if "argmax" in got:
    assert bool(torch.equal(got["argmax"], s["argmax"])), "%s: %sarg-max is not the first maximum of the kernel's own logits in %d pixels" % (
        wt.tag, pre, int((got["argmax"] != s["argmax"]).sum()))
  return s


def _judge_forward(wt, pre, got, ref, D):
  wt.inside(pre + "logits", got["logits"], ref["logits"], ref["e_logits"])
  _judge_soft(wt, pre, got, D)
  ok = tr.decided(ref["logits"], ref["e_logits"])
  share = 1.0 - float(ok.double().mean())
  assert share < tr.UNDECIDED_CAP, "%s: %.2f %% of the pixels undecided" % (wt.tag, 100 * share)
  if "argmax" in got:
    bad = (got["argmax"] != torch.argmax(ref["logits"], 1)) & ok
    assert not bool(bad.any()), "%s: %sarg-max differs from the reference's in %d decided pixels" % (wt.tag, pre, int(bad.sum()))
  return share


def _same_bits(a, b, what):
  torch.cuda.synchronize()
  for n in ("logits", "pred", "am", "fcs"):
    fa, fb = getattr(a, n), getattr(b, n)
    if fa is not None and fb is not None:
      assert bool(torch.equal(fa.raw, fb.raw)), "%s: %s differs in %d words" % (what, n, int((fa.raw != fb.raw).sum()))


def _a_out_buf(g):
  """the by-product's destination: a zero halo around an interior of PATTERN"""
  return PclBuf(g, None, "zero")


@pytest.mark.parametrize("geom,npos", tr.FWD_GEOMS, ids=["%s-%dpos" % (tr.geom_id(g), n) for g, n in tr.FWD_GEOMS])
def test_fused_tail_forward(geom, npos):
  """as_agg_tail_fwd on agg_tail_direct_kernel<.., 16> and <.., 32> (the XCD tile bijection at grids of 2, 9, 513 and above; one tile
  exactly; the last tile shifted back; D = 1, 2, 3, 8, 9, 32; W = 173), the three input flavours, and the first-generation pair
  of launches on the same input."""
  lib = nat.load()
  B, D, H, W = geom
  g = Pcl(B, D, H, W, 1, 1, 1)
  assert lib.as_agg_tail_ok(g) == 1 and lib.as_agg_tail_fwd_positions(g) == npos == tr.fwd_route(geom), (lib.as_agg_tail_fwd_positions(g), npos)
  wt = Worst("fwd %s %d positions" % (tr.geom_id(geom), npos))
  x_buf, share = None, 0.0
  for gain in tr.GAINS:
    c = tr.fwd_case(geom, gain)
    x_buf = x_buf or PclBuf(g, c["x"])                       # (the same x at every gain)
    w, b, sc, sh = _dev(c["w"]), _dev(c["b"]), _dev(c["scale"]), _dev(c["shift"])
    # IN 0: x is the activated volume
    ref = tr.forward(c["x"], c["w"], c["b"])
    o0 = _tail(x_buf, g, w, b)
    share = max(share, _judge_forward(wt, "", o0.read("as_agg_tail_fwd"), ref, D))
    # the first generation on the same input, against the same references
    o1 = _first_generation(x_buf, g, w, b)
    _judge_forward(wt, "first generation ", o1.read("as_conv3d_out_fwd + as_softargmax_fwd"), ref, D)
    # IN 1: the raw volume with the BatchNorm affine + LeakyReLU on the way in, with and without the by-product
    ref = tr.forward(c["x"], c["w"], c["b"], c["scale"], c["shift"])
    a_out = _a_out_buf(g)
    o2 = _tail(x_buf, g, w, b, sc, sh, a_out=a_out)
    share = max(share, _judge_forward(wt, "affine ", o2.read("as_agg_tail_fwd (affine)"), ref, D))
    wt.inside("a_out", a_out.interior("a_out"), ref["a"], ref["e_a"])
    o3 = _tail(x_buf, g, w, b, sc, sh)
    _same_bits(o3, o2, "affine input without the by-product")
    if geom in tr.FWD_ONCE and gain == 50.0:
      # IN 2: the BatchNorm still in partials, equal bit for bit to IN 1 with the state it finalised
      gen = torch.Generator().manual_seed(21)
      parts = ops.StatParts(37, DEV)
      parts.mean.copy_((torch.randn(37 * 32, generator=gen) * 0.3).to(DEV))
      parts.m2.copy_((torch.randn(37 * 32, generator=gen).abs() * 50 + 5).to(DEV))
      parts.cnt.copy_((torch.randn(37, generator=gen).abs() * 90 + 10).floor().to(DEV))
      parts.cnt[5] = 0.0
      parts.m2[5 * 32:6 * 32] = 0.0
      gam, bet = _dev(torch.randn(32, generator=gen) * 0.5 + 1.0), _dev(torch.randn(32, generator=gen) * 0.2)
      pa = ops.PendingBn(parts, gam, bet, torch.zeros(32, device=DEV), torch.ones(32, device=DEV))
      a_m, a_a = _a_out_buf(g), _a_out_buf(g)
      o_m = _tail(x_buf, g, w, b, in_bn=pa, a_out=a_m)
      o_a = _tail(x_buf, g, w, b, pa.state.scale, pa.state.shift, a_out=a_a)
      _same_bits(o_m, o_a, "BatchNorm in partials against its finalised affine")
      assert bool(torch.equal(a_m.interior("a_out (partials)"), a_a.interior("a_out (affine)")))
      # NULL bias, arg-max and FCS
      refn = tr.forward(c["x"], c["w"], None)
      o_n = _tail(x_buf, g, w, None)
      _judge_forward(wt, "no bias ", o_n.read("as_agg_tail_fwd (no bias)"), refn, D)
      o_p = _tail(x_buf, g, w, None, want_argmax=False, want_fcs=False)
      _same_bits(o_p, o_n, "NULL argmax and fcs")
      o_p.read("as_agg_tail_fwd (NULL argmax, fcs)")
  if geom in tr.FWD_TAP_GEOMS:
    xt = None
    for t in range(27):
      c = tr.tap_case(geom, t)
      xt = xt or PclBuf(g, c["x"])
      got = _tail(xt, g, _dev(c["w"]), _dev(c["b"])).read("as_agg_tail_fwd single tap %d" % t)
      wt.exact("logits single tap %d" % t, got["logits"], tr.logits_sum(c["x"], c["w"], c["b"]))
      _judge_soft(wt, "single tap ", got, D)
  if geom in tr.FWD_DESIGNED_GEOMS:
    c = tr.designed_case(geom, npos)
    got = _tail(PclBuf(g, c["x"]), g, _dev(c["w"]), None).read("as_agg_tail_fwd designed logits")
    wt.exact("designed logits", got["logits"], c["l"])
    s = _judge_soft(wt, "designed ", got, D)
    assert bool(torch.equal(got["argmax"], torch.argmax(c["l"], 1)))
    assert bool(torch.isfinite(got["pred"]).all()) and bool(torch.isfinite(got["fcs"]).all())
    for (name, tag), (bi, y, x) in sorted(c["where"].items()):
      assert int(got["argmax"][bi, y, x]) == int(s["argmax"][bi, y, x]), (name, tag)
  wt.note(grid=tr.fwd_grid(geom), undecided_share=round(share, 5))


@pytest.mark.parametrize("geom", tr.FWD_REFUSED, ids=tr.geom_id)
def test_fused_tail_refuses(geom):
  """W = 174, D = 33 and npos = 31: as_agg_tail_ok == 0, the query answers 0 and the entry point refuses before any launch"""
  lib = nat.load()
  B, D, H, W = geom
  g = Pcl(B, D, H, W, 1, 1, 1)
  assert tr.fwd_route(geom) == 0 and lib.as_agg_tail_ok(g) == 0 and lib.as_agg_tail_fwd_positions(g) == 0
  x = torch.zeros(g.numel(), device=DEV)
  w = torch.zeros(32 * 27, device=DEV)
  o = TailOut(g)
  rc = lib.as_agg_tail_fwd(nat.ptr(x), g, None, None, None, None, nat.ptr(w), None, SLOPE, o.logits.ptr(), o.pred.ptr(), o.am.ptr(),
                           o.fcs.ptr(), nat.stream())
  assert rc != 0 and b"geometry" in lib.as_last_error()
  assert bool((o.logits.guards_kept("refused") == PATTERN).all())


# ----------------------------------------------------------------------------- the backward
def _tail_bwd(g, logits, g_pred, g_in, a_buf, w, gw0, gb0):
  lib = nat.load()
  acc = 1 if gw0 is not None else 0
  n_ws = lib.as_agg_tail_bwd_workspace(g)
  ws, g_a = Flat(n_ws), PclBuf(g, None, "pattern")
  g_w, g_b = Flat(864, gw0), Flat(1, gb0)
  nat.call("as_agg_tail_bwd", nat.ptr(logits), nat.ptr(g_pred), nat.ptr(g_in), a_buf.ptr(), g, nat.ptr(w), g_a.ptr(), g_w.ptr(), g_b.ptr(),
           acc, ws.ptr(), nat.stream())
  ws.guards_kept("as_agg_tail_bwd workspace")
  return g_a.interior("as_agg_tail_bwd g_a"), g_w.result("as_agg_tail_bwd g_w").view(32, 3, 3, 3), g_b.result("as_agg_tail_bwd g_bias")


def _three_launches(g, logits, g_pred, g_in, a_buf, w, gw0, gb0):
  lib = nat.load()
  acc = 1 if gw0 is not None else 0
  gl = Flat(g.B * g.D * g.H * g.W)
  nat.call("as_softargmax_bwd", nat.ptr(logits), nat.ptr(g_pred), nat.ptr(g_in), g.B, g.D, g.H, g.W, gl.ptr(), nat.stream())
  ws, g_a = Flat(lib.as_conv3d_out_bwd_workspace(g)), PclBuf(g, None, "pattern")
  g_w, g_b = Flat(864, gw0), Flat(1, gb0)
  nat.call("as_conv3d_out_bwd", gl.ptr(), a_buf.ptr(), g, nat.ptr(w), g_a.ptr(), g_w.ptr(), g_b.ptr(), acc, ws.ptr(), nat.stream())
  ws.guards_kept("as_conv3d_out_bwd workspace")
  return (gl.result("as_softargmax_bwd g_logits").view(g.B, g.D, g.H, g.W), g_a.interior("as_conv3d_out_bwd g_a"),
          g_w.result("as_conv3d_out_bwd g_w").view(32, 3, 3, 3), g_b.result("as_conv3d_out_bwd g_bias"))


FLAVOURS = {"g_pred + g_in": (1, 1), "g_pred": (1, 0), "g_in": (0, 1)}


def _bwd_combos(geom):
  if geom[0] * geom[1] * geom[2] * geom[3] <= SMALL:
    return [(k, f, acc) for k in tr.GAINS for f in FLAVOURS for acc in (0, 1)]
  return [(1.0, "g_pred + g_in", 0), (50.0, "g_pred", 1), (300.0, "g_in", 0), (50.0, "g_pred + g_in", 1)]


def _bwd_random(wt, geom, g, launch, pre=""):
  a_buf = None
  for gain, flavour, acc in _bwd_combos(geom):
    c = tr.bwd_case(geom, gain)
    a_buf = a_buf or PclBuf(g, c["a"], "pattern")             # (the same activation at every gain; its halo must not be consumed)
    gp, gi = FLAVOURS[flavour]
    kw = dict(g_pred=c["g_pred"] if gp else None, g_in=c["g_in"] if gi else None, gw0=c["gw0"] if acc else None,
              gb0=c["gb0"] if acc else None)
    ref = tr.tail_backward(c["logits"], c["a"], c["w"], **kw)
    logits, gpd, gid = _dev(c["logits"]), _dev(kw["g_pred"]), _dev(kw["g_in"])
    got = launch(g, logits, gpd, gid, a_buf, _dev(c["w"]), kw["gw0"], kw["gb0"])
    tag = pre + (" accumulate" if acc else "")
    if len(got) == 4:
      wt.inside("g_logits" + pre, got[0], ref["gl"], ref["e_gl"])
      got = got[1:]
    wt.inside("g_a" + pre, got[0], ref["g_a"], ref["e_g_a"])
    wt.inside("g_w" + tag, got[1], ref["g_w"], ref["e_g_w"])
    wt.inside("g_bias" + tag, got[2], ref["g_b"], ref["e_g_b"])


@pytest.mark.parametrize("geom,xc", tr.BWD_GEOMS, ids=["%s-%dcol" % (tr.geom_id(g), n) for g, n in tr.BWD_GEOMS])
def test_fused_tail_backward(geom, xc):
  """as_agg_tail_bwd on agg_tail_bwd_kernel<13> and <26>: W = 1, D = 1 and 32, one full chunk, a chunk of one column, W below the
  chunk width, the unit count exactly on 768, and workgroups that walk two units on either flavour."""
  lib = nat.load()
  B, D, H, W = geom
  g = Pcl(B, D, H, W, 1, 1, 1)
  assert lib.as_agg_tail_bwd_ok(g) == 1 and lib.as_agg_tail_bwd_columns(g) == xc == tr.bwd_route(geom), (lib.as_agg_tail_bwd_columns(g), xc)
  wt = Worst("bwd %s %d columns" % (tr.geom_id(geom), xc))
  _bwd_random(wt, geom, g, _tail_bwd)
  if geom in tr.BWD_EXACT_GEOMS:
    small = B * D * H * W <= SMALL
    for t in (range(27) if small else (0, 13, 26)):
      for spot in (tr.BWD_SPOTS if small else [tr.BWD_SPOTS[t % 2]]):
        c = tr.bwd_exact_case(geom, t, spot, xc)
        acc = (t + (spot == "seam")) % 2
        gw0, gb0 = (c["gw0"], c["gb0"]) if acc else (None, None)
        ref = tr.tail_backward(c["logits"], c["a"], c["w"], None, c["g_in"], gw0, gb0)
        got = _tail_bwd(g, _dev(c["logits"]), None, _dev(c["g_in"]), PclBuf(g, c["a"], "pattern"), _dev(c["w"]), gw0, gb0)
        what = "tap %d, impulses at the %s%s" % (t, spot, ", accumulate" if acc else "")
        wt.exact("g_a " + what, got[0], ref["g_a"])
        wt.exact("g_w " + what, got[1], ref["g_w"])
        wt.exact("g_bias " + what, got[2], ref["g_b"])
  wt.note(units=tr.bwd_units(geom))


@pytest.mark.parametrize("geom", tr.BWD_FIRST_GEN_GEOMS, ids=tr.geom_id)
def test_three_launch_backward(geom):
  """as_softargmax_bwd + as_conv3d_out_bwd (the fallback where as_agg_tail_bwd_ok == 0) against the same references: the logits
  gradient it stores, and g_a, g_w, g_bias end to end; 9 x 12 x 24 x 78 reaches the caps of 4096 blocks and 512 slabs."""
  B, D, H, W = geom
  g = Pcl(B, D, H, W, 1, 1, 1)
  wt = Worst("bwd three launches %s" % tr.geom_id(geom))
  _bwd_random(wt, geom, g, _three_launches, " (three launches)")
  wt.note(blocks=min((B * D * H * W + 31) // 32, 4096))


# ----------------------------------------------------------------------------- the cost volume
@pytest.mark.parametrize("geom", tr.CV_GEOMS, ids=tr.geom_id)
def test_cost_volume_and_its_adjoint(geom):
  """as_cost_volume_fwd: the correctly rounded difference, bit for bit, zeros at x < d included, the halo untouched;
  as_cost_volume_bwd against float64 with gamma(terms of the column), the gradient's halo (PATTERN) never consumed.  D = 64 > W,
  W = 16 exactly, W % 16 == 15, and one voxel."""
  B, D, H, W = geom
  g = Pcl(B, D, H, W, 1, 1, 1)
  c = tr.cv_case(geom)
  wt = Worst("cost volume %s" % tr.geom_id(geom))
  L, R = Flat(B * 32 * H * W, c["L"]), Flat(B * 32 * H * W, c["R"])
  vol = PclBuf(g, None, "pattern")
  nat.call("as_cost_volume_fwd", L.ptr(), R.ptr(), vol.ptr(), g, nat.stream())
  wt.exact("vol", vol.interior("as_cost_volume_fwd"), tr.cost_volume(c["L"], c["R"], D))
  gvol = PclBuf(g, c["gvol"], "pattern")
  gL, gR = Flat(B * 32 * H * W), Flat(B * 32 * H * W)
  nat.call("as_cost_volume_bwd", gvol.ptr(), gL.ptr(), gR.ptr(), g, nat.stream())
  ref = tr.cost_volume_bwd(c["gvol"])
  wt.inside("gL", gL.result("as_cost_volume_bwd gL").view(B, 32, H, W), ref["gL"], ref["e_gL"])
  wt.inside("gR", gR.result("as_cost_volume_bwd gR").view(B, 32, H, W), ref["gR"], ref["e_gR"])
  wt.note()
