"""The 2-D row-segment 32 -> 32 kernels (csrc/conv32_lds.hip) through the C ABI, ONE LAUNCH AT A TIME, against float64 and the
derived bounds of tests/lds2d_ref.py (held to torch, to the library's route queries and to eight mutants by
tests/test_lds2d_ref_cpu.py): as_conv32_fwd (MODE 0 with moments, with and without a residual; MODE 2 with and without a
residual; epilogue 1 plain, with a foreign residual and with residual == x, which is conv32_lds_skip_kernel),
as_conv32_fwd_bnbwd (MODE 3 with a residual and with residual = NULL), as_conv32_wgrad (conv32_wgrad_lds_kernel and, from 3072
tiles on, conv32_wgrad_lds2_kernel) and as_conv32_wgrad_bnapply.

Geometries (lds2d_ref.forward_cases): (1, 3, 128) three tiles on a grid of 8 — five workgroups own nothing and must still publish
(0, 0, 0) partials, zero sums and zero slabs; (1, 5, 129) a second segment shifted to x0 = 1 that keeps ONE column; (1, 9, 160)
duplicates ending on a wave boundary; (2, 7, 255), (1, 6, 256), (1, 2, 257) dup = 1, no shift, three segments with row indices
crossing an image; (3, 29, 770) 609 tiles on 512 workgroups, a short last band.  Dilations 1, 2, 4, 8 on the first three, 3 and 7
on (1, 5, 129) and (3, 29, 770); halo rows = d (the least accepted) and halo columns 8, one case with halo (8, 12) at d = 2 and one
whose output halo (3, 9) differs from its input's (1, 8).  The weight gradient also at (1, 3071, 128) (the last size on
conv32_wgrad_lds_kernel), (3, 1024, 128) (3072 tiles: conv32_wgrad_lds2_kernel, one workgroup walks 12 tiles through both
buffers), (4, 384, 129) (the same with a one-column second segment, plain and as as_conv32_wgrad_bnapply, accumulate 0 and 1) and
with output pw = 7, which must leave the LDS route (as_conv32_wgrad_segments != 0).  Below W = 128 the same entry points fall
through to split-K ((1, 9, 127), d = 2) and the direct kernel ((3, 100, 127), d = 1) of conv32_mfma.hip and to the generic weight
gradient: moments, eval + residual and the weight gradient are judged there too.  Every case first asserts its route through
the read-only queries.

Buffers: outputs, their halos, the partials and the slab workspaces start as one NaN bit pattern between guard words: every
interior word must be overwritten, every halo and guard word must keep the pattern.  Inputs sit in ZEROED halos between NaN
guards: that is the production contract (the pool hands out zeroed buffers and no kernel writes a halo), and the weight gradient
depends on it — its clamped DMA bases read the row's right halo as the zero g_z beyond W, and what a clamped X group fetches only
ever multiplies that zero.

Families: random with +-1e4 sentinels on the first and last rows and columns of every input; a common offset of 1e3 on the bias
(the moments' pivot); the exact integer family (nine single-tap weights and a dense one) in which z, eval, g_x, the next sums,
g_z, dW, db and accumulate = 1 equal float64 bit for bit.  Moments and next sums are judged PER PARTIAL against float64 of the
kernel's own stored output over the pixels the owner map gives that workgroup; counts are exact.  No element is left out except
those undecided on a LeakyReLU branch (the next sums, stage 3), which are counted, capped at 1e-4 of the case and judged against
the nearer branch.  The float64 references run on the card.  The worst err / bound of every output goes to
conftest.parity_note (lds2d[...]).

Worst err / bound seen on an MI355X.  as_conv32_fwd on the LDS kernels (21 geometries, both families): z 0.085 (with a residual
0.083), moments mean 0.30 and M2 0.023 (3 x 29 x 770), g_x of MODE 2 0.033 (with a residual 0.034), eval 0.086, + residual 0.085,
+ skip 0.085.  as_conv32_fwd_bnbwd: g_x 0.034 with a residual and 0.033 with residual = NULL, both with MODE 2's bits; next sums
0.36 and 0.35.  as_conv32_wgrad: dW 0.17 and db 0.023 (accumulating 0.026 and 0.010); at 3071 tiles 0.013 / 0.0016, at 3072 tiles
0.019 / 0.0028 and 0.024 / 0.0038 (one-column segment); output pw = 7 (generic kernel) 0.0082 / 0.0016.
as_conv32_wgrad_bnapply: g_z 0.68 (an element-wise chain: every rounding at half an ulp) with as_bn_act_bwd's bits, dW 0.035,
db 0.020, the same accumulating.  Below 128 columns: z 0.084, eval + residual 0.083, mean 0.18, M2 0.24, dW 0.012, db 0.0010.
Undecided elements: none on y_next or y in any case.  All 20 exact cases (ten weights each) and the exact
as_conv32_wgrad_bnapply were bit-exact, the largest sum at 0.0037 * 2^24 quanta; the five idle workgroups of (1, 3, 128)
published (0, 0, 0), zero sums and zero slabs; every route assertion held and nothing was found wrong in csrc/: MODE 3 with
residual = NULL is right in this build.  The file takes 8.4 s: 48 cases, the slowest 1.6 s (the first one, which loads the
library) and 1.5 s ((4, 384, 129), five weight-gradient launches with their float64 references).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from adaptive_stereo import _native as nat
from adaptive_stereo import hip_ops as ops
from adaptive_stereo.hip_ops import Pcl, ConvShape
import lds2d_ref as lr
from conftest import parity_note

DEV = "cuda:0"
PATTERN = 0x7FF92345        # a quiet NaN that no arithmetic produces
GUARD = 64
SLAB = 9 * 1024 + 32


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
  """a channel-last input [B, H, W, 32] inside a ZERO halo, between guard floats of PATTERN"""

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
    r = lr.ratio(got, ref, bound)
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
    parity_note("lds2d[%s]" % self.tag, **extra, **self.extra, **{"worst_err_over_bound_" + k: v for k, v in self.r.items()})


def _same_bits(a, b, what):
  torch.cuda.synchronize()
  assert bool(torch.equal(a.raw, b.raw)), "%s differ in %d words" % (what, int((a.raw != b.raw).sum()))


# ----------------------------------------------------------------------------- one launch each
class Layer(object):
  """the geometries, the packed filters and the staged inputs of one case"""

  def __init__(self, c4, k):
    (B, H, W), d, hin, hout = c4
    self.c4, self.k, self.d = c4, k, d
    self.gin, self.gout, self.shape = Pcl(B, 1, H, W, 0, *hin), Pcl(B, 1, H, W, 0, *hout), _shape(d)
    self.wp, self.wp_t = ops.pack_weights(k["w"], self.shape, False), ops.pack_weights(k["w"], self.shape, True)
    self.bufs = {}

  def route(self, fwd, wgrad):
    """asserts the restated routes and the library's queries name the kernels this case is here for"""
    lib = nat.load()
    (B, H, W), d, hin, hout = self.c4
    assert lr.fwd_route(B, H, W, d, hin) == fwd and lr.wgrad_route(B, H, W, d, hin, hout) == wgrad
    assert lib.as_conv32_stat_parts(self.gin, self.gout, self.shape) == lr.stat_parts(B, H, W, d, hin)
    assert lib.as_conv32_bnbwd_parts(self.gin, self.gout, self.shape) == lr.bnbwd_parts(B, H, W, d, hin)
    assert lib.as_conv32_wgrad_bnapply_ok(self.gin, self.gout, self.shape) == (1 if wgrad == "lds2" else 0)
    seg, ws = lib.as_conv32_wgrad_segments(self.gin, self.gout, self.shape), lib.as_conv32_wgrad_workspace(self.gin, self.gout, self.shape)
    if wgrad == "generic":
      assert seg >= 1 and ws % SLAB == 0
    else:
      assert seg == 0 and ws == lr.wgrad_workspace(B, H, W, d, hin, hout)
    self.parts, self.slabs = lr.stat_parts(B, H, W, d, hin), ws // SLAB

  def inp(self, name, g):
    key = (name, g.key())
    if key not in self.bufs:
      self.bufs[key] = InBuf(self.k[name], g)
    return self.bufs[key]

  def fwd(self, x, transposed=False, bias=False, epilogue=0, residual=None, moments=False):
    """as_conv32_fwd; x / residual name tensors of the case (the residual in the output geometry; residual == x: the same buffer)"""
    k, gi, go = self.k, self.gin, self.gout
    z = OutBuf(go)
    st = [Flat(self.parts * 32), Flat(self.parts * 32), Flat(self.parts)] if moments else [None, None, None]
    res = None if residual is None else (self.inp(x, gi) if residual == x else self.inp(residual, go))
    nat.call("as_conv32_fwd", self.inp(x, gi).ptr(), gi, nat.ptr(self.wp_t if transposed else self.wp), nat.ptr(k["b"]) if bias else None,
             z.ptr(), go, self.shape, epilogue, nat.ptr(k["st"]["scale"]) if epilogue else None,
             nat.ptr(k["st"]["shift"]) if epilogue else None, k["slope"], res.ptr() if res else None,
             *[s.ptr() if s else None for s in st], nat.stream())
    return z, st

  def bnbwd(self, residual):
    k, gi, go = self.k, self.gin, self.gout
    sn = k["st_next"]
    gx, sums = OutBuf(go), Flat(self.parts * 128)
    nat.call("as_conv32_fwd_bnbwd", self.inp("g_a", gi).ptr(), gi, nat.ptr(self.wp_t), gx.ptr(), go, self.shape,
             self.inp(residual, go).ptr() if residual else None, self.inp("z_next", go).ptr(), nat.ptr(sn["scale"]), nat.ptr(sn["shift"]),
             nat.ptr(sn["mean"]), k["slope"], sums.ptr(), nat.stream())
    return gx, sums

  def wgrad(self, accumulate, dW0=None, db0=None):
    ws, dW, db = Flat(self.slabs * SLAB), Flat(9216, dW0), Flat(32, db0)
    nat.call("as_conv32_wgrad", self.inp("x", self.gin).ptr(), self.gin, self.inp("g_a", self.gout).ptr(), self.gout, self.shape, dW.ptr(),
             db.ptr(), accumulate, ws.ptr(), nat.stream())
    return dW.result("as_conv32_wgrad dW").view(32, 32, 3, 3), db.result("as_conv32_wgrad db"), ws.result("as_conv32_wgrad workspace")

  def bnapply(self, coef, accumulate, dW0=None, db0=None):
    k, st = self.k, self.k["st"]
    ws, dW, db, gz = Flat(self.slabs * SLAB), Flat(9216, dW0), Flat(32, db0), OutBuf(self.gout)
    nat.call("as_conv32_wgrad_bnapply", self.inp("x", self.gin).ptr(), self.gin, self.inp("g_a", self.gout).ptr(), self.inp("z", self.gout).ptr(),
             self.gout, self.shape, nat.ptr(st["scale"]), nat.ptr(st["shift"]), nat.ptr(st["mean"]), nat.ptr(coef), k["slope"], gz.ptr(),
             dW.ptr(), db.ptr(), accumulate, ws.ptr(), nat.stream())
    ws.result("as_conv32_wgrad_bnapply workspace")
    return gz, dW.result("as_conv32_wgrad_bnapply dW").view(32, 32, 3, 3), db.result("as_conv32_wgrad_bnapply db")


def _acc_init(integers=False):
  gen = torch.Generator().manual_seed(77)
  if integers:
    return torch.randint(-8, 9, (32, 32, 3, 3), generator=gen).float(), torch.randint(-8, 9, (32,), generator=gen).float()
  return torch.randn(32, 32, 3, 3, generator=gen), torch.randn(32, generator=gen)


def _judge_wgrad(wt, ly, route, dW, db, accumulate, tag=""):
  k = ly.k
  d0, b0 = _acc_init() if accumulate else (None, None)
  wg = lr.weight_gradient(k["x"], k["g_a"], ly.d, route, ly.slabs, d0, b0)
  tag += " accumulate" if accumulate else ""
  wt.inside("dW" + tag, dW, wg["dW"], wg["e_dW"])
  wt.inside("db" + tag, db, wg["db"], wg["e_db"])


# ----------------------------------------------------------------------------- the LDS kernels, bounded families
CASES = lr.forward_cases()


@pytest.mark.parametrize("c4", CASES, ids=[lr.case_id(c) for c in CASES])
def test_every_launch_against_float64(c4):
  """both bounded families through every forward flavour, MODE 3 with and without a residual, and the weight gradient (random:
  set, offset: accumulating)"""
  (B, H, W), d, hin, hout = c4
  n = B * H * W * 32
  same_halo = hin == hout
  for fam in ("random", "offset"):
    k = lr.case((B, H, W), d, fam, DEV)
    ly = Layer(c4, k)
    ly.route("lds2d", "lds")
    wt = Worst("%s %s" % (lr.case_id(c4), fam))
    w, sl, st, sn = k["w"], k["slope"], k["st"], k["st_next"]
    grid = ly.parts
    assert grid == lr.conv32_lds_grid(B, H, W)
    own = lr.owner_map(B, H, W, grid, DEV)
    n_l = 16 * lr.most_tiles(lr.ntiles(B, H, W), grid)
    # ---- MODE 0: raw output + moments, then the same with a residual (the moments are the accumulator's: equal bits)
    z, ms = ly.fwd("x", bias=True, moments=True)
    z32 = z.interior("as_conv32_fwd z")
    f = lr.forward_z(k["x"], w, k["b"], d)
    wt.inside("z", z32, f["z"], f["e_z"])
    m = lr.moments(z32, own, grid, n_l)
    assert bool(torch.equal(ms[2].result("moments count").double(), m["cnt"])), "%s: a partial's count is not its owned pixels" % wt.tag
    wt.inside("mean", ms[0].result("moments mean").view(grid, 32), m["mean"], m["e_mean"])
    wt.inside("M2", ms[1].result("moments M2").view(grid, 32), m["m2"], m["e_m2"])
    z2, ms2 = ly.fwd("x", bias=True, residual="a_pp", moments=True)
    f = lr.forward_z(k["x"], w, k["b"], d, residual=k["a_pp"])
    wt.inside("z + residual", z2.interior("as_conv32_fwd z + residual"), f["z"], f["e_z"])
    for a, b_, what in zip(ms, ms2, ("mean", "M2", "count")):
      _same_bits(a, b_, "moments (%s) with and without a residual" % what)
    del z, z2, ms, ms2, f, m
    # ---- MODE 2: the data gradient, with and without a residual in the output geometry
    gx2, _ = ly.fwd("g_a", transposed=True, residual="a_pp")
    f = lr.forward_z(k["g_a"], w, None, d, residual=k["a_pp"], transposed=True)
    wt.inside("g_x (MODE 2) + residual", gx2.interior("as_conv32_fwd g_x + residual"), f["z"], f["e_z"])
    gx0, _ = ly.fwd("g_a", transposed=True)
    f0 = lr.forward_z(k["g_a"], w, None, d, transposed=True)
    wt.inside("g_x (MODE 2)", gx0.interior("as_conv32_fwd g_x"), f0["z"], f0["e_z"])
    # ---- epilogue 1: plain, a foreign residual, residual == x (the skip read from the staged centre row)
    for res, rt, name in ((None, None, "eval"), ("a_pp", k["a_pp"], "eval + residual"), ("x", k["x"], "eval + skip")):
      if res == "x" and not same_halo:
        continue                                             # (residual == x is a residual in the INPUT geometry)
      out, _ = ly.fwd("x", bias=True, epilogue=1, residual=res)
      e = lr.eval_out(k["x"], w, k["b"], st["scale"], st["shift"], sl, rt, d)
      wt.inside(name, out.interior("as_conv32_fwd " + name), e["out"], e["e_out"])
    del out, e
    # ---- MODE 3: the data gradient + stage 1 of the next BatchNorm backward; g_x has MODE 2's bits
    for res, ref, twin in (("a_pp", f, gx2), (None, f0, gx0)):
      name = " + residual" if res else ", residual NULL"
      gx, sums = ly.bnbwd(res)
      gx32 = gx.interior("as_conv32_fwd_bnbwd g_x" + name)
      wt.inside("g_x (MODE 3)" + name, gx32, ref["z"], ref["e_z"])
      _same_bits(gx, twin, "g_x of MODE 3 and of MODE 2" + name)
      ns = lr.next_sums(gx32, k["z_next"], sn["scale"], sn["shift"], sn["mean"], sl, own, grid, n_l)
      wt.undecided("y_next", ns["undecided"], n)
      wt.inside("next sums" + name, sums.result("next sums" + name, torch.float64).view(grid, 64), ns["sums"], ns["e_sums"])
    del gx, gx0, gx2, sums, ns, f, f0
    # ---- the weight gradient
    acc = 0 if fam == "random" else 1
    dW, db, ws = ly.wgrad(acc, *(_acc_init() if acc else (None, None)))
    _judge_wgrad(wt, ly, "lds", dW, db, acc)
    idle = [b for b in range(ly.slabs) if len(lr.wg_tiles(b, lr.ntiles(B, H, W), ly.slabs)) == 0]
    for b in idle:                                           # a workgroup without a tile publishes a zero slab
      assert not bool(ws[b * 9216:(b + 1) * 9216].any()) and not bool(ws[ly.slabs * 9216 + 32 * b:ly.slabs * 9216 + 32 * b + 32].any()), \
          "%s: the slab of idle workgroup %d is not zero" % (wt.tag, b)
    wt.note(tiles=lr.ntiles(B, H, W), grid=grid, slabs=ly.slabs, idle_slabs=len(idle))
    del ly
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- the exact integer family
@pytest.mark.parametrize("c4", lr.EXACT_CASES, ids=[lr.case_id(c) for c in lr.EXACT_CASES])
def test_integer_cases_are_exact(c4):
  """small-integer operands, slope 0.5, scales that are powers of two: every launch must equal float64 bit for bit, for each of
  the nine single-tap weights and a dense one; the headroom (every sum of absolute terms below 2^24 quanta) is asserted"""
  (B, H, W), d, hin, hout = c4
  wt = Worst("%s exact" % lr.case_id(c4))
  d0, b0 = _acc_init(integers=True)
  room = 0.0
  for wfam in lr.EXACT_WEIGHTS:
    k = lr.exact_case((B, H, W), d, wfam, DEV)
    ly = Layer(c4, k)
    ly.route("lds2d", "lds")
    w, sl, st, sn, name = k["w"], k["slope"], k["st"], k["st_next"], "%s %d" % wfam
    grid = ly.parts
    own = lr.owner_map(B, H, W, grid, DEV)
    f = lr.forward_z(k["x"], w, k["b"], d)
    z, ms = ly.fwd("x", bias=True, moments=True)
    wt.exact("z " + name, z.interior("z"), f["z"])
    assert bool(torch.equal(ms[2].result("count").double(), lr.moments(z.interior("z"), own, grid, 16)["cnt"]))
    for res, rt in (("x", k["x"]), ("a_pp", k["a_pp"]), (None, None)):
      out, _ = ly.fwd("x", bias=True, epilogue=1, residual=res)
      wt.exact("eval %s %s" % (res, name), out.interior("eval"), lr.eval_out(k["x"], w, k["b"], st["scale"], st["shift"], sl, rt, d)["out"])
    g = lr.forward_z(k["g_a"], w, None, d, residual=k["a_pp"], transposed=True)
    gx2, _ = ly.fwd("g_a", transposed=True, residual="a_pp")
    wt.exact("g_x (MODE 2) " + name, gx2.interior("g_x"), g["z"])
    gx, sums = ly.bnbwd("a_pp")
    wt.exact("g_x (MODE 3) " + name, gx.interior("g_x"), g["z"])
    ns = lr.next_sums(gx.interior("g_x"), k["z_next"], sn["scale"], sn["shift"], sn["mean"], sl, own, grid, 16)
    wt.exact("next sums " + name, sums.result("next sums", torch.float64).view(grid, 64), ns["sums"])
    gx, sums = ly.bnbwd(None)
    wt.exact("g_x (MODE 3, NULL) " + name, gx.interior("g_x"), lr.conv_direct(k["g_a"], w, d, transposed=True))
    room = max(room, lr.exact_headroom(2 * f["S"] + 2, g["S"]))
    if wfam[0] == "dense":                                   # (the weight gradient has no weights: once)
      dWr, dbr = lr.wgrad_direct(k["x"], k["g_a"], d)
      room = max(room, lr.exact_headroom(*[s + 8 for s in lr.wgrad_direct(k["x"].abs(), k["g_a"].abs(), d)]))
      dW, db, _ = ly.wgrad(0)
      wt.exact("dW", dW, dWr)
      wt.exact("db", db, dbr)
      dW, db, _ = ly.wgrad(1, d0, b0)
      wt.exact("dW accumulate", dW, dWr + d0.double().to(DEV))
      wt.exact("db accumulate", db, dbr + b0.double().to(DEV))
    del ly
  assert room < 2 ** 24, "%s: a sum may reach %.3g quanta: the case is not exact in fp32" % (wt.tag, room)
  wt.note(largest_sum_over_2p24=room / 2 ** 24)
  torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- the weight gradient at the switch of its kernels
@pytest.mark.parametrize("c4", lr.WGRAD_LARGE, ids=[lr.case_id(c) for c in lr.WGRAD_LARGE])
def test_weight_gradient_either_side_of_3072_tiles(c4):
  """3071 tiles stay on conv32_wgrad_lds_kernel (192 slabs), 3072 take conv32_wgrad_lds2_kernel (256 slabs, 12 tiles per
  workgroup); (4, 384, 129) also as as_conv32_wgrad_bnapply: g_z written inside only, judged against float64 and equal to
  as_bn_act_bwd's bits, dW / db element by element, accumulate 0 and 1, and once more on the exact integer family"""
  (B, H, W), d, hin, hout = c4
  lib = nat.load()
  route = "lds2" if lr.wgrad_lds2(B, H, W) else "lds"
  assert route == ("lds" if (B, H, W) == (1, 3071, 128) else "lds2")
  k = lr.case((B, H, W), d, "random", DEV)
  ly = Layer(c4, k)
  ly.route("lds2d", route)
  assert ly.slabs == lr.conv32_wgrad_lds_slabs(B, H, W) == (192 if route == "lds" else 256)
  wt = Worst("%s random" % lr.case_id(c4))
  dW, db, _ = ly.wgrad(0)
  _judge_wgrad(wt, ly, route, dW, db, 0)
  if W % lr.SEG:
    n = B * H * W * 32
    st, sl, g = k["st"], k["slope"], ly.gout
    # stages 1 and 2 of the BatchNorm backward leave the coefficients k1, k2, k3 in the workspace (g_z = NULL) ...
    ws = torch.empty(lib.as_bn_bwd_workspace(g), device=DEV)
    invstd, gam = torch.full((32,), 0.75, device=DEV), torch.linspace(0.5, 1.5, 32, device=DEV)
    gg, gb = torch.zeros(32, device=DEV), torch.zeros(32, device=DEV)
    bn = lambda gz: nat.call("as_bn_act_bwd", ly.inp("g_a", g).ptr(), ly.inp("z", g).ptr(), nat.ptr(st["scale"]), nat.ptr(st["shift"]),
                             nat.ptr(st["mean"]), nat.ptr(invstd), nat.ptr(gam), sl, 1, gz, nat.ptr(gg), nat.ptr(gb), 0, nat.ptr(ws), g,
                             nat.stream())
    bn(None)
    coef = ws[lib.as_bn_bwd_coef_offset():lib.as_bn_bwd_coef_offset() + 96].clone()
    ref = lr.gz_chain(k["g_a"], k["z"], st["scale"], st["shift"], st["mean"], coef, sl)
    # ... stage 3 as its own pass, for the bits
    gz_sep = torch.zeros(g.numel(), device=DEV)
    bn(nat.ptr(gz_sep))
    gz_sep = ops.pcl_view(gz_sep, g)[:, 0, g.ph:g.ph + H, g.pw:g.pw + W]
    for acc in (0, 1):
      gz, dW, db = ly.bnapply(coef, acc, *(_acc_init() if acc else (None, None)))
      gz32 = gz.interior("as_conv32_wgrad_bnapply g_z")
      r, und = lr.judge_gz(gz32, ref)
      wt.undecided("y", und, n)
      wt.ratio("g_z", r)
      assert bool(torch.equal(gz32, gz_sep)), "stage 3 on the staged row differs from as_bn_act_bwd's in %d elements" % int((gz32 != gz_sep).sum())
      # (dW from the launch's own g_z)
      d0, b0 = _acc_init() if acc else (None, None)
      wg = lr.weight_gradient(k["x"], gz32, d, route, ly.slabs, d0, b0)
      tag = " accumulate" if acc else ""
      wt.inside("bnapply dW" + tag, dW, wg["dW"], wg["e_dW"])
      wt.inside("bnapply db" + tag, db, wg["db"], wg["e_db"])
      del wg, gz
    # the exact family: k1 = k2 = 0, k3 = 2
    ke = lr.exact_case((B, H, W), d, ("dense", 0), DEV)
    le = Layer(c4, ke)
    le.route("lds2d", route)
    d0, b0 = _acc_init(integers=True)
    gz, dW, db = le.bnapply(ke["coef"], 1, d0, b0)
    gzr = lr.gz_chain(ke["g_a"], ke["z"], ke["st"]["scale"], ke["st"]["shift"], ke["st"]["mean"], ke["coef"], ke["slope"])["g_z"]
    gz32 = gz.interior("g_z (exact)")
    wt.exact("g_z", gz32, gzr)
    dWr, dbr = lr.wgrad_direct(ke["x"], gz32, d)
    room = lr.exact_headroom(*[s + 8 for s in lr.wgrad_direct(ke["x"].abs(), gz32.abs(), d)])
    assert room < 2 ** 24
    wt.exact("bnapply dW accumulate", dW, dWr + d0.double().to(DEV))
    wt.exact("bnapply db accumulate", db, dbr + b0.double().to(DEV))
  wt.note(tiles=lr.ntiles(B, H, W), slabs=ly.slabs)
  torch.cuda.empty_cache()


def test_weight_gradient_leaves_the_lds_route_below_8_output_halo_columns():
  """output pw = 7: a G group beyond W would read the next row, so the entry point must take the generic kernel
  (as_conv32_wgrad_segments != 0) — and the result is still right"""
  c4 = lr.WGRAD_NARROW_HALO
  (B, H, W), d, _, _ = c4
  for fam, acc in (("random", 0), ("offset", 1)):
    ly = Layer(c4, lr.case((B, H, W), d, fam, DEV))
    ly.route("lds2d", "generic")
    wt = Worst("%s %s" % (lr.case_id(c4), fam))
    dW, db, _ = ly.wgrad(acc, *(_acc_init() if acc else (None, None)))
    _judge_wgrad(wt, ly, "generic", dW, db, acc)
    wt.note(slabs=ly.slabs)


# ----------------------------------------------------------------------------- below W = 128: split-K, the direct kernel, the generic weight gradient
@pytest.mark.parametrize("c4", lr.BELOW_128, ids=[lr.case_id(c) for c in lr.BELOW_128])
def test_the_same_entry_points_below_128_columns(c4):
  (B, H, W), d, hin, hout = c4
  fwd = "splitk" if B * H * W <= lr.SPLITK_MAX_M else "direct"
  assert fwd == ("splitk" if (B, H, W) == (1, 9, 127) else "direct")
  per = 32 if fwd == "splitk" else 128
  for fam, acc in (("random", 0), ("offset", 1)):
    k = lr.case((B, H, W), d, fam, DEV)
    ly = Layer(c4, k)
    ly.route(fwd, "generic")
    wt = Worst("%s %s %s" % (lr.case_id(c4), fwd, fam))
    parts = ly.parts
    assert parts == -(-B * H * W // per)
    z, ms = ly.fwd("x", bias=True, moments=True)
    z32 = z.interior("as_conv32_fwd z")
    f = lr.forward_z(k["x"], k["w"], k["b"], d)
    wt.inside("z", z32, f["z"], f["e_z"])
    m = lr.moments_two_pass(z32, lr.flat_owner(B, H, W, per, DEV), parts)
    assert bool(torch.equal(ms[2].result("moments count").double(), m["cnt"]))
    wt.inside("mean", ms[0].result("moments mean").view(parts, 32), m["mean"], m["e_mean"])
    wt.inside("M2", ms[1].result("moments M2").view(parts, 32), m["m2"], m["e_m2"])
    out, _ = ly.fwd("x", bias=True, epilogue=1, residual="a_pp")
    e = lr.eval_out(k["x"], k["w"], k["b"], k["st"]["scale"], k["st"]["shift"], k["slope"], k["a_pp"], d)
    wt.inside("eval + residual", out.interior("as_conv32_fwd eval + residual"), e["out"], e["e_out"])
    dW, db, _ = ly.wgrad(acc, *(_acc_init() if acc else (None, None)))
    _judge_wgrad(wt, ly, "generic", dW, db, acc)
    wt.note(parts=parts, slabs=ly.slabs)
    del ly
  torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- refusals
def test_entry_points_refuse_what_the_queries_decline():
  """as_conv32_fwd_bnbwd where as_conv32_bnbwd_parts == 0 and as_conv32_wgrad_bnapply below 3072 tiles: the argument error,
  as_last_error set, every output word kept"""
  lib = nat.load()
  # stage 1 of the BatchNorm backward exists in the LDS kernel alone: W = 127
  c4 = lr.BELOW_128[0]
  (B, H, W), d, hin, hout = c4
  k = lr.case((B, H, W), d, "random", DEV)
  ly = Layer(c4, k)
  assert lib.as_conv32_bnbwd_parts(ly.gin, ly.gout, ly.shape) == 0
  gx, sums = OutBuf(ly.gout), Flat(512 * 128)
  sn = k["st_next"]
  rc = lib.as_conv32_fwd_bnbwd(ly.inp("g_a", ly.gin).ptr(), ly.gin, nat.ptr(ly.wp_t), gx.ptr(), ly.gout, ly.shape, None,
                               ly.inp("z_next", ly.gout).ptr(), nat.ptr(sn["scale"]), nat.ptr(sn["shift"]), nat.ptr(sn["mean"]), k["slope"],
                               sums.ptr(), nat.stream())
  msg = lib.as_last_error().decode()
  assert rc == -1 and "as_conv32_fwd_bnbwd" in msg and "not supported" in msg, (rc, msg)
  gx.untouched("as_conv32_fwd_bnbwd g_x")
  sums.untouched("as_conv32_fwd_bnbwd sums")
  # stage 3 exists in the chip-filling weight gradient alone: 10 tiles, and one tile short of 3072
  for c4 in (lr._c4((1, 5, 129), 1), lr.WGRAD_LARGE[0]):
    (B, H, W), d, hin, hout = c4
    k = dict(lr.case((1, 5, 129), 1, "random", DEV))
    g = Pcl(B, 1, H, W, 0, *hin)
    shape = _shape(d)
    assert lib.as_conv32_wgrad_bnapply_ok(g, g, shape) == 0 and lr.ntiles(B, H, W) < lr.LDS2_TILES
    x = torch.zeros(g.numel(), device=DEV)
    ws, dW, db, gz = Flat(lib.as_conv32_wgrad_workspace(g, g, shape)), Flat(9216), Flat(32), OutBuf(g)
    st = k["st"]
    rc = lib.as_conv32_wgrad_bnapply(nat.ptr(x), g, nat.ptr(x), nat.ptr(x), g, shape, nat.ptr(st["scale"]), nat.ptr(st["shift"]),
                                     nat.ptr(st["mean"]), nat.ptr(k["coef"]), k["slope"], gz.ptr(), dW.ptr(), db.ptr(), 0, ws.ptr(),
                                     nat.stream())
    msg = lib.as_last_error().decode()
    assert rc == -1 and "as_conv32_wgrad_bnapply" in msg and "not supported" in msg, (rc, msg)
    for b in (ws, dW, db, gz):
      b.untouched("as_conv32_wgrad_bnapply at %d tiles" % lr.ntiles(B, H, W))
