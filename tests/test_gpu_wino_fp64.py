"""The minimal-filtering kernels of the refinement's six dilated 32 -> 32 layers through the C ABI, ONE LAUNCH AT A TIME, against the
float64 restatement and the derived bounds of tests/wino_ref.py (held to torch on the CPU, and shown to tell twelve mutants from
the right restatement, by tests/test_wino_ref_cpu.py): as_conv32_wino_fwd, as_conv32_wino_eval, as_conv32_wino_bwd_data (both
generations), as_conv32_wino_bwd_filter and as_conv32_wino_bwd_fused, as_conv32_wino_pack_weights through them.

Geometries: for every dilation the six of wino_ref.geometries — exactly 2048 units (the acceptance floor; one image fewer is
declined), a lone row in comb 0 with a neighbour segment that keeps ONE column, three segments, combs of different lengths with
a neighbour that keeps 63 columns, W a multiple of 64, and 23 + d x 191 — each with the smallest batch the query accepts, halo
rows = d (the least the query accepts) and halo columns 8.  Every case asserts as_conv32_wino_ok == 1 and which data-gradient
generation runs; the two generations must write equal bits.

Buffers: outputs, their halos, the moment / sum partials and both slab workspaces start as one NaN bit pattern between guard
words: every interior word must be overwritten, every halo and guard word must keep the pattern.  Inputs sit in zeroed halos
between NaN guards.  g_z is judged in a pattern-halo buffer and copied into a zero-halo buffer for as_conv32_wino_bwd_filter.

Families: random with +-1e4 sentinels on the first and last rows and columns of every input; a common offset of 1e3 on z_prev and
the bias (the moments' pivot); on the first three geometries of every dilation the exact integer family (nine single-tap
weights and a dense one), where every output — z, a_out, eval, g_z, g_x, the next sums, dW, db, accumulate = 1 on an integer
dW — equals float64 bit for bit.  The moments and the next BatchNorm's sums are judged PER PARTIAL against float64 over the
pixels the restated tiling gives that workgroup, of the kernel's own fp32 output; dW and db element by element against float64
from the two-launch g_z.  The float64 references run on the card (the same wino_ref code).  No element is left out except those
undecided on a LeakyReLU branch, which are counted, capped at 1e-4 of the case and judged against the nearer branch.  The worst
err / bound of every output goes to conftest.parity_note (wino[...]).

Worst err / bound seen on an MI355X over the 24 geometries and both families: a_out 0.985 and g_z 0.937 (element-wise chains:
every rounding at half an ulp), z 0.023, eval 0.023, g_x 0.027, moments mean 0.36 (offset family, 53 x 25 x 191, d = 2) and M2
0.036, next sums 0.15 (fused 0.20), dW 0.016 and db 0.034 (fused, accumulating 0.027 and 0.077; 5e-5 and 1e-3 in the offset
family).  Undecided elements: at most 1 on y and 1 on y_next per case (8 to 17 million elements).  Every exact case was
bit-exact, its largest accumulator below 0.028 * 2^24 quanta; the two data-gradient generations and the fused launch's g_x gave
equal bits everywhere.  Found: as_conv32_wino_bwd accepted gin != gout (it hands gout alone to both launches, so x in another
padded geometry was read with the wrong strides) — it now asks the query like its five siblings.  The file takes 84 s: 24 cases
of 2 to 3.3 s, 12 exact cases of 3.6 to 5.5 s (ten weights each), 7 refusals.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from adaptive_stereo import _native as nat
from adaptive_stereo.hip_ops import Pcl, ConvShape
import wino_ref as wr
from conftest import parity_note

DEV = "cuda:0"
PATTERN = 0x7FF92345        # a quiet NaN that no arithmetic produces
GUARD = 64
PW = 8


def _shape(d):
  return ConvShape(1, 3, 3, 0, d, d, d, 1)


# ----------------------------------------------------------------------------- buffers
class OutBuf(object):
  """an output with a halo (PCL: [B, H + 2 ph, W + 2 pw, 32]), every word PATTERN"""

  def __init__(self, g):
    self.g = g
    self.raw = torch.full((GUARD + g.numel() + GUARD,), PATTERN, dtype=torch.int32, device=DEV)

  def ptr(self):
    return nat.ptr(self.raw[GUARD:])

  def untouched(self, what):
    torch.cuda.synchronize()
    assert bool((self.raw == PATTERN).all()), "%s: a refused launch wrote %d words" % (what, int((self.raw != PATTERN).sum()))

  def interior(self, what):
    """the interior as fp32 (on the card); asserts guards and halo kept, interior overwritten"""
    torch.cuda.synchronize()
    g, r = self.g, self.raw
    assert bool((r[:GUARD] == PATTERN).all()) and bool((r[-GUARD:] == PATTERN).all()), "%s: wrote outside the tensor" % what
    v = r[GUARD:-GUARD].view(g.B, g.H + 2 * g.ph, g.W + 2 * g.pw, 32)
    inner = v[:, g.ph:g.ph + g.H, g.pw:g.pw + g.W]
    nhalo = int((v != PATTERN).sum()) - int((inner != PATTERN).sum())
    assert nhalo == 0, "%s: %d halo words were written" % (what, nhalo)
    f = inner.contiguous().view(torch.float32)
    nn = int(torch.isnan(f).sum())
    assert nn == 0, "%s: %d interior elements are NaN (not written, or a guard value was consumed)" % (what, nn)
    return f


class InBuf(object):
  """a channel-last input [B, H, W, 32] inside a zero halo, between guard floats of PATTERN"""

  def __init__(self, t, g):
    p = F.pad(t.float(), (0, 0, g.pw, g.pw, g.ph, g.ph)).reshape(-1)
    self.raw = torch.full((GUARD + p.numel() + GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    self.raw[GUARD:GUARD + p.numel()].view(torch.float32).copy_(p)

  def ptr(self):
    return nat.ptr(self.raw[GUARD:])


class Flat(object):
  """numel 4-byte words of output inside a buffer of PATTERN; `init` (fp32) for an accumulating launch"""

  def __init__(self, numel, init=None):
    self.n = numel
    self.raw = torch.full((GUARD + numel + GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    if init is not None:
      self.raw[GUARD:GUARD + numel].view(torch.float32).copy_(init.reshape(-1).to(DEV))

  def ptr(self):
    return nat.ptr(self.raw[GUARD:])

  def untouched(self, what):
    torch.cuda.synchronize()
    assert bool((self.raw == PATTERN).all()), "%s: a refused launch wrote %d words" % (what, int((self.raw != PATTERN).sum()))

  def result(self, what, dtype=torch.float32):
    torch.cuda.synchronize()
    r = self.raw
    assert bool((r[:GUARD] == PATTERN).all()) and bool((r[-GUARD:] == PATTERN).all()), \
        "%s: wrote outside the destination (partials beyond the launch's own)" % what
    body = r[GUARD:GUARD + self.n]
    assert not bool((body == PATTERN).any()), "%s: %d words not written" % (what, int((body == PATTERN).sum()))
    v = body.view(dtype)
    assert not bool(torch.isnan(v).any()), "%s: %d NaN" % (what, int(torch.isnan(v).sum()))
    return v


class Worst(object):
  def __init__(self, tag):
    self.tag, self.r, self.extra = tag, {}, {}

  def inside(self, name, got, ref, bound):
    r = wr.ratio(got, ref, bound)
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
    assert count <= 1e-4 * numel, "%s: %d of %d elements undecided on %s" % (self.tag, count, numel, name)

  def note(self, **extra):
    parity_note("wino[%s]" % self.tag, **extra, **self.extra, **{"worst_err_over_bound_" + k: v for k, v in self.r.items()})


def _same_bits(a, b, what):
  torch.cuda.synchronize()
  assert bool(torch.equal(a.raw, b.raw)), "%s differ in %d words" % (what, int((a.raw != b.raw).sum()))


# ----------------------------------------------------------------------------- one launch each
class Layer(object):
  """the geometry, the packed filters and the staged inputs of one case"""

  def __init__(self, geom, d, c):
    lib = nat.load()
    B, H, W = geom
    self.geom, self.d, self.c = geom, d, c
    self.g, self.shape = Pcl(B, 1, H, W, 0, d, PW), _shape(d)
    assert lib.as_conv32_wino_ok(self.g, self.g, self.shape) == 1
    assert wr.units(B, H, W, d) >= 2048 > wr.units(B - 1, H, W, d)
    self.ww, self.ww_t = torch.empty(16 * 1024, device=DEV), torch.empty(16 * 1024, device=DEV)
    nat.call("as_conv32_wino_pack_weights", nat.ptr(c["w"]), nat.ptr(self.ww), 0, nat.stream())
    nat.call("as_conv32_wino_pack_weights", nat.ptr(c["w"]), nat.ptr(self.ww_t), 1, nat.stream())
    self.bufs = {}

  def inp(self, name):
    if name not in self.bufs:
      self.bufs[name] = InBuf(self.c[name], self.g)
    return self.bufs[name]

  def forward(self, skip, moments, bias=True):
    lib, c, g = nat.load(), self.c, self.g
    parts = lib.as_conv32_wino_parts()
    a_out, z = OutBuf(g), OutBuf(g)
    st = [Flat(parts * 32), Flat(parts * 32), Flat(parts)] if moments else [None, None, None]
    nat.call("as_conv32_wino_fwd", self.inp("z_prev").ptr(), self.inp("a_pp").ptr() if skip else None, nat.ptr(c["st_in"]["scale"]),
             nat.ptr(c["st_in"]["shift"]), a_out.ptr(), g, nat.ptr(self.ww), nat.ptr(c["b"]) if bias else None, c["slope"], z.ptr(),
             g, self.shape, *[s.ptr() if s else None for s in st], nat.stream())
    return a_out, z, st, parts

  def eval(self, residual, bias):
    c, g = self.c, self.g
    out = OutBuf(g)
    nat.call("as_conv32_wino_eval", self.inp("x").ptr(), g, self.shape, nat.ptr(self.ww), nat.ptr(c["b"]) if bias else None,
             nat.ptr(c["st"]["scale"]), nat.ptr(c["st"]["shift"]), c["slope"], residual, out.ptr(), nat.stream())
    return out

  def _bwd_args(self):
    c = self.c
    return (nat.ptr(c["st"]["scale"]), nat.ptr(c["st"]["shift"]), nat.ptr(c["st"]["mean"]), nat.ptr(c["coef"]), c["slope"],
            self.inp("z_next").ptr(), nat.ptr(c["st_next"]["scale"]), nat.ptr(c["st_next"]["shift"]), nat.ptr(c["st_next"]["mean"]))

  def data(self, generation):
    """as_conv32_wino_bwd_data under a generation setting; returns g_z, g_x, the sums buffer, its partial count"""
    lib, g = nat.load(), self.g
    parts = lib.as_conv32_wino_bwd_parts()
    gz, gx, sums = OutBuf(g), OutBuf(g), Flat(parts * 128)
    prev = lib.as_conv32_wino_bwd_generation(0)
    try:
      lib.as_conv32_wino_bwd_generation(generation)
      assert lib.as_conv32_wino_bwd_generation(0) == generation
      nat.call("as_conv32_wino_bwd_data", self.inp("g_a").ptr(), self.inp("z").ptr(), g, self.shape, nat.ptr(self.ww_t),
               *self._bwd_args(), gz.ptr(), gx.ptr(), sums.ptr(), nat.stream())
      torch.cuda.synchronize()
    finally:
      lib.as_conv32_wino_bwd_generation(prev)
    return gz, gx, sums, parts

  def filter(self, gz32, accumulate, dW0=None, db0=None):
    lib, g = nat.load(), self.g
    ws = Flat(lib.as_conv32_wino_bwd_workspace())
    dW, db = Flat(9216, dW0), Flat(32, db0)
    gz_in = InBuf(gz32, g)                                   # (the header requires a zero halo here)
    nat.call("as_conv32_wino_bwd_filter", self.inp("x").ptr(), gz_in.ptr(), g, self.shape, dW.ptr(), db.ptr(), accumulate, ws.ptr(),
             nat.stream())
    ws.result("as_conv32_wino_bwd_filter workspace")
    return dW.result("as_conv32_wino_bwd_filter dW").view(32, 32, 3, 3), db.result("as_conv32_wino_bwd_filter db")

  def fused(self, accumulate, dW0=None, db0=None):
    lib, g = nat.load(), self.g
    parts = lib.as_conv32_wino_bwd_fused_parts()
    ws = Flat(lib.as_conv32_wino_bwd_fused_workspace())
    gx, sums, dW, db = OutBuf(g), Flat(parts * 128), Flat(9216, dW0), Flat(32, db0)
    nat.call("as_conv32_wino_bwd_fused", self.inp("x").ptr(), g, self.inp("g_a").ptr(), self.inp("z").ptr(), g, self.shape,
             nat.ptr(self.ww_t), *self._bwd_args(), gx.ptr(), dW.ptr(), db.ptr(), accumulate, sums.ptr(), ws.ptr(), nat.stream())
    ws.result("as_conv32_wino_bwd_fused workspace")
    return gx, sums, parts, dW.result("as_conv32_wino_bwd_fused dW").view(32, 32, 3, 3), db.result("as_conv32_wino_bwd_fused db")


def _generations(d):
  """(the setting that is the default, the kernel it runs; the other kernel's setting)"""
  lib = nat.load()
  assert lib.as_conv32_wino_bwd_generation(0) == 2            # the default: conv32_wino_dgrad.hip for d <= 4, MODE 2 for d = 8
  return (2, 1) if d <= 4 else (2, 3)


GEOMS = [(g, d) for d in wr.DILATIONS for g in wr.geometries(d)]
IDS = ["%s-d%d" % (wr.geom_id(g), d) for g, d in GEOMS]


# ----------------------------------------------------------------------------- the bounded families
@pytest.mark.parametrize("geom,d", GEOMS, ids=IDS)
def test_every_launch_against_float64(geom, d):
  """random (sentinels): forward with skip and moments, inference block with residual and bias, both data-gradient generations,
  the weight gradient set, the fused backward accumulating; offset: forward without skip, with moments and with all three NULL
  (equal bits), inference block plain without bias, the default data gradient, the weight gradient accumulating, the fused
  backward set."""
  B, H, W = geom
  n = B * H * W * 32
  for fam in ("random", "offset"):
    c = wr.case(geom, d, fam, DEV)
    ly = Layer(geom, d, c)
    wt = Worst("%s d%d %s" % (wr.geom_id(geom), d, fam))
    rnd, sl, w = fam == "random", c["slope"], c["w"]
    # ---- forward
    a_out, z, st, parts = ly.forward(skip=rnd, moments=True)
    a32 = a_out.interior("as_conv32_wino_fwd a_out")
    a_ref, e_a = wr.act_chain(c["z_prev"], c["a_pp"] if rnd else None, c["st_in"]["scale"], c["st_in"]["shift"], sl)
    wt.inside("a_out", a32, a_ref, e_a)
    z32 = z.interior("as_conv32_wino_fwd z")
    f = wr.forward_z(a32, w, c["b"], d)
    wt.inside("z", z32, f["z"], f["e_z"])
    m = wr.moments(z32, d, parts)
    assert bool(torch.equal(st[2].result("moments count").double(), m["cnt"])), "%s: a partial's count is not its owned pixels" % wt.tag
    wt.inside("mean", st[0].result("moments mean").view(parts, 32), m["mean"], m["e_mean"])
    wt.inside("M2", st[1].result("moments M2").view(parts, 32), m["m2"], m["e_m2"])
    del f, m, a_ref, e_a
    if not rnd:
      a2, z2, _, _ = ly.forward(skip=False, moments=False)
      _same_bits(z2, z, "z with and without the moment arrays")
      _same_bits(a2, a_out, "a_out with and without the moment arrays")
      del a2, z2
    del a_out, z, st
    # ---- inference block
    out = ly.eval(1 if rnd else 0, bias=rnd)
    e = wr.eval_out(c["x"], w, c["b"] if rnd else None, c["st"]["scale"], c["st"]["shift"], sl, rnd, d)
    wt.inside("eval", out.interior("as_conv32_wino_eval"), e["out"], e["e_out"])
    del out, e
    # ---- data gradient
    default, other = _generations(d)
    gz, gx, sums, parts = ly.data(default)
    if rnd:
      gz_o, gx_o, sums_o, _ = ly.data(other)
      _same_bits(gz_o, gz, "g_z of the two generations")
      _same_bits(gx_o, gx, "g_x of the two generations")
      _same_bits(sums_o, sums, "next sums of the two generations")
      del gz_o, gx_o, sums_o
    gz32, gx32 = gz.interior("as_conv32_wino_bwd_data g_z"), gx.interior("as_conv32_wino_bwd_data g_x")
    r, und = wr.judge_gz(gz32, wr.gz_chain(c["g_a"], c["z"], c["st"]["scale"], c["st"]["shift"], c["st"]["mean"], c["coef"], sl))
    wt.undecided("y", und, n)
    wt.ratio("g_z", r)
    dg = wr.data_gradient(gz32, c["g_a"], w, d)
    wt.inside("g_x", gx32, dg["g_x"], dg["e_g_x"])
    del dg
    sn = c["st_next"]
    ns = wr.next_sums(gx32, c["z_next"], sn["scale"], sn["shift"], sn["mean"], sl, d, parts)
    wt.undecided("y_next", ns["undecided"], n)
    wt.inside("next sums", sums.result("next sums", torch.float64).view(parts, 64), ns["sums"], ns["e_sums"])
    # ---- weight gradient (its own partition: 256 slabs, no shifted segment)
    slabs = nat.load().as_conv32_wino_bwd_workspace() // (9 * 1024 + 32)
    gen = torch.Generator().manual_seed(77)
    d0, b0 = torch.randn(32, 32, 3, 3, generator=gen), torch.randn(32, generator=gen)
    acc = 0 if rnd else 1
    dW, db = ly.filter(gz32, acc, d0 if acc else None, b0 if acc else None)
    wg = wr.weight_gradient(c["x"], gz32, d, slabs, False, d0 if acc else None, b0 if acc else None, slabs=slabs)
    tag = " accumulate" if acc else ""
    wt.inside("dW" + tag, dW, wg["dW"], wg["e_dW"])
    wt.inside("db" + tag, db, wg["db"], wg["e_db"])
    # ---- the whole backward in one launch: g_x equal bits, dW on its own against float64 from the two-launch g_z
    acc = 1 - acc
    gx_f, sums_f, fparts, dW, db = ly.fused(acc, d0 if acc else None, b0 if acc else None)
    _same_bits(gx_f, gx, "g_x of the fused launch and of the two launches")
    wg = wr.weight_gradient(c["x"], gz32, d, fparts, True, d0 if acc else None, b0 if acc else None, slabs=fparts)
    tag = " accumulate" if acc else ""
    wt.inside("fused dW" + tag, dW, wg["dW"], wg["e_dW"])
    wt.inside("fused db" + tag, db, wg["db"], wg["e_db"])
    ns = wr.next_sums(gx32, c["z_next"], sn["scale"], sn["shift"], sn["mean"], sl, d, fparts)
    wt.inside("fused next sums", sums_f.result("fused next sums", torch.float64).view(fparts, 64), ns["sums"], ns["e_sums"])
    wt.note(units=wr.units(B, H, W, d))
    del ly, gz, gx, sums, gx_f, sums_f, wg, ns
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- the exact integer family
EXACT = [(g, d) for d in wr.DILATIONS for g in wr.geometries(d)[:3]]


@pytest.mark.parametrize("geom,d", EXACT, ids=["%s-d%d" % (wr.geom_id(g), d) for g, d in EXACT])
def test_integer_cases_are_exact(geom, d):
  """small-integer operands, slope 0.5, scales that are powers of two, k1 = k2 = 0, k3 = 2: every launch must equal float64 bit
  for bit, element by element, for each of the nine single-tap weights and a dense one; the precondition (every accumulator's
  sum|terms| below 2^24 quanta) is asserted on the case before it is judged."""
  B, H, W = geom
  wt = Worst("%s d%d exact" % (wr.geom_id(geom), d))
  gen = torch.Generator().manual_seed(78)
  d0, b0 = torch.randint(-8, 9, (32, 32, 3, 3), generator=gen).float(), torch.randint(-8, 9, (32,), generator=gen).float()
  default, other = _generations(d)
  room = 0.0
  for wfam in wr.EXACT_WEIGHTS:
    c = wr.exact_case(geom, d, wfam, DEV)
    ly = Layer(geom, d, c)
    sl, w, name = c["slope"], c["w"], "%s %d" % wfam
    dense = wfam[0] == "dense"
    # forward
    a_out, z, _, _ = ly.forward(skip=True, moments=dense)
    a32, z32 = a_out.interior("a_out"), z.interior("z")
    wt.exact("a_out " + name, a32, wr.act_chain(c["z_prev"], c["a_pp"], c["st_in"]["scale"], c["st_in"]["shift"], sl)[0])
    assert bool(torch.equal(a32 * 4, (a32 * 4).round()))
    room = max(room, wr.exact_headroom(a32, w, d, 0.25, 1.0))
    wt.exact("z " + name, z32, wr.conv_direct(a32, w, d) + c["b"].double())
    del a_out, z, a32, z32
    # inference block
    room = max(room, 2 * wr.exact_headroom(c["x"], w, d, 1.0, 1.0))
    out = ly.eval(1, bias=True)
    wt.exact("eval " + name, out.interior("eval"), wr.eval_out(c["x"], w, c["b"], c["st"]["scale"], c["st"]["shift"], sl, 1, d)["out"])
    del out
    # data gradient
    gz, gx, sums, parts = ly.data(default if wfam[1] % 2 == 0 else other)
    gz32, gx32 = gz.interior("g_z"), gx.interior("g_x")
    wt.exact("g_z " + name, gz32, wr.gz_chain(c["g_a"], c["z"], c["st"]["scale"], c["st"]["shift"], c["st"]["mean"], c["coef"], sl)["g_z"])
    assert bool(torch.equal(gz32, gz32.round()))
    room = max(room, wr.exact_headroom(gz32, w, d, 1.0, 1.0, transposed=True))
    wt.exact("g_x " + name, gx32, wr.conv_direct(gz32, w, d, transposed=True) + c["g_a"].double())
    sn = c["st_next"]
    ns = wr.next_sums(gx32, c["z_next"], sn["scale"], sn["shift"], sn["mean"], sl, d, parts)
    wt.exact("next sums " + name, sums.result("next sums", torch.float64).view(parts, 64), ns["sums"])
    # weight gradient: the stand-alone launch set, the fused launch accumulating on an integer dW
    room = max(room, wr.exact_headroom_wgrad(c["x"], gz32, d, 1.0, 1.0, False), wr.exact_headroom_wgrad(c["x"], gz32, d, 1.0, 1.0, True))
    dWr, dbr = wr.wgrad_direct(c["x"], gz32, d)
    dW, db = ly.filter(gz32, 0)
    wt.exact("dW " + name, dW, dWr)
    wt.exact("db " + name, db, dbr)
    gx_f, sums_f, fparts, dW, db = ly.fused(1, d0, b0)
    _same_bits(gx_f, gx, "g_x of the fused launch and of the two launches")
    wt.exact("fused dW accumulate " + name, dW, dWr + d0.double().to(DEV))
    wt.exact("fused db accumulate " + name, db, dbr + b0.double().to(DEV))
    ns = wr.next_sums(gx32, c["z_next"], sn["scale"], sn["shift"], sn["mean"], sl, d, fparts)
    wt.exact("fused next sums " + name, sums_f.result("fused next sums", torch.float64).view(fparts, 64), ns["sums"])
    del ly, gz, gx, sums, gx_f, sums_f
  assert room < 2 ** 24, "%s: an accumulator may reach %.3g quanta: the case is not exact in fp32" % (wt.tag, room)
  wt.note(largest_accumulator_over_2p24=room / 2 ** 24)
  torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- refusals
def _refusals():
  ok = lambda d: dict(B=2048 // d, H=2 * d, W=64, d=d, ph=d, pw=PW)
  out = [("W 63", dict(ok(1), W=63)), ("H 2d - 1", dict(ok(2), H=3, B=1024)), ("dilation 3", dict(ok(1), d=3, ph=3, H=6)),
         ("2047 units", dict(ok(1), B=2047)), ("halo columns 7", dict(ok(1), pw=7)), ("halo rows d - 1", dict(ok(2), ph=1)),
         ("gin != gout", dict(ok(1), out_pw=9))]
  return out


@pytest.mark.parametrize("what,k", _refusals(), ids=[w for w, _ in _refusals()])
def test_entry_points_refuse_what_the_query_declines(what, k):
  """as_conv32_wino_ok returns 0 (or the argument error) and all six entry points return the argument error before any launch:
  every word of the pattern-filled outputs is kept.  The buffers have the full size of the declared geometry."""
  lib = nat.load()
  d = k["d"]
  g = Pcl(k["B"], 1, k["H"], k["W"], 0, k["ph"], k["pw"])
  go = Pcl(k["B"], 1, k["H"], k["W"], 0, k["ph"], k.get("out_pw", k["pw"]))
  shape = _shape(d)
  assert lib.as_conv32_wino_ok(g, go, shape) in (0, -1), what
  if "out_pw" not in k and what != "halo rows d - 1":
    assert lib.as_conv32_wino_ok(g, g, shape) == 0
  big = Pcl(k["B"], 1, k["H"], k["W"], 0, k["ph"], max(k["pw"], k.get("out_pw", 0)))
  x = torch.zeros(big.numel(), device=DEV)
  vec, coef, wq = torch.ones(32, device=DEV), torch.ones(96, device=DEV), torch.zeros(16 * 1024, device=DEV)
  outs = [OutBuf(big), OutBuf(big)]
  small = [Flat(lib.as_conv32_wino_parts() * 32), Flat(lib.as_conv32_wino_parts() * 32), Flat(lib.as_conv32_wino_parts()),
           Flat(9216), Flat(32), Flat(lib.as_conv32_wino_bwd_parts() * 128), Flat(lib.as_conv32_wino_bwd_workspace()),
           Flat(lib.as_conv32_wino_bwd_fused_workspace())]
  mean, m2, cnt, dW, db, sums, ws, wsf = small
  P, s = nat.ptr, nat.stream()
  bwd = (P(vec), P(vec), P(vec), P(coef), ctypes.c_float(0.2), P(x), P(vec), P(vec), P(vec))
  calls = {
      "as_conv32_wino_fwd": lambda: lib.as_conv32_wino_fwd(P(x), None, P(vec), P(vec), outs[0].ptr(), g, P(wq), P(vec), 0.2, outs[1].ptr(),
                                                           go, shape, mean.ptr(), m2.ptr(), cnt.ptr(), s),
      "as_conv32_wino_bwd": lambda: lib.as_conv32_wino_bwd(P(x), g, P(x), P(x), go, shape, P(wq), *bwd, outs[0].ptr(), outs[1].ptr(),
                                                           dW.ptr(), db.ptr(), 0, sums.ptr(), ws.ptr(), s),
      "as_conv32_wino_bwd_fused": lambda: lib.as_conv32_wino_bwd_fused(P(x), g, P(x), P(x), go, shape, P(wq), *bwd, outs[1].ptr(),
                                                                       dW.ptr(), db.ptr(), 0, sums.ptr(), wsf.ptr(), s),
  }
  if "out_pw" not in k:                                     # (these take ONE geometry)
    calls.update({
        "as_conv32_wino_eval": lambda: lib.as_conv32_wino_eval(P(x), g, shape, P(wq), P(vec), P(vec), P(vec), 0.2, 1, outs[0].ptr(), s),
        "as_conv32_wino_bwd_data": lambda: lib.as_conv32_wino_bwd_data(P(x), P(x), g, shape, P(wq), *bwd, outs[0].ptr(), outs[1].ptr(),
                                                                       sums.ptr(), s),
        "as_conv32_wino_bwd_filter": lambda: lib.as_conv32_wino_bwd_filter(P(x), P(x), g, shape, dW.ptr(), db.ptr(), 0, ws.ptr(), s),
    })
  for name, fn in calls.items():
    rc = fn()
    msg = lib.as_last_error().decode()
    assert rc == -1, "%s accepted %s (status %d)" % (name, what, rc)
    if what != "halo rows d - 1":                            # (that one already fails the generic reach check: another message)
      assert "not supported" in msg, "%s refused %s with: %s" % (name, what, msg)
  for b in outs + small:
    b.untouched(what)
