"""as_upsample_bilinear_fwd / _bwd (csrc/resample.hip) through the C ABI against the float64 reference and the bound of
tests/resample_ref.py (held to torch on the CPU by tests/test_resample_ref_cpu.py).  Every destination is a slice of a larger
buffer pre-filled with one NaN bit pattern: after the launch no NaN is left inside (everything was written) and every word
around it is bit-unchanged (nothing was written outside; the forward's first vector piece of a misaligned row deliberately
starts before the row).  No element is excluded from a comparison.  The worst error / bound of every case goes to
conftest.parity_note.

What the cases are for, by kernel path:
  forward   LDS flavour and the non-LDS one (source rows wider than 1024; a w = 1024 / 1025 pair straddles the switch), a second
            pass of the X0 loop (W > 4096), destination bases off a 16-byte boundary by 1, 2, 3 floats, rows shorter than a
            vector, workgroups of four rows that straddle two images (the staged source rows must be refilled; h = 1 is the
            case where the row indices alone do not change), identity (bit-exact), constant and corner sources.
  backward  the production shapes (chunk clamped to w at 131 <- 17, a ragged last chunk at 960 <- 60 and 1242 <- 156), all-ones
            gradients (every term positive: a dropped tap shows), single-pixel gradients on the first and last fine index of
            coarse rows' and columns' support and at the corners, more than 256 footprint rows (no row-weight table) and exactly
            256 / 257 of them, chunk == 1, the adjoint of a down-sampling, the refusal of a ratio beyond UPB_SPAN, determinism.

What the numbers look like, and why.  The forward sits at 0.2 .. 0.4 of its bound, almost all of it the coordinate term (the
kernel contracts the coordinate into one fma, the reference does not).  The dense backward sits at 0.01 .. 0.1: K counts every
addition of a sequential sum at its worst, while the roundings of ~32 terms of either sign mostly cancel; all-ones gradients
(no cancellation) reach 0.04 .. 0.07 and single-pixel gradients 0.23.  Two changes to the kernels that these tests cannot see,
both because they change no value beyond the reference's own uncertainty: footprint() with its slack of 1 removed and one index
tighter (floor(lower) + 1 is the first fine index strictly inside the support; tests/test_resample_ref_cpu.py shows that what
the slack still guards are weights inside the coordinate allowance; one index tighter again fails 16 tests here), and the
row-weight table used up to 255 instead of 256 rows (the path without the table adds the same products in the same order).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from adaptive_stereo import _native as nat
import resample_ref as rr
from conftest import parity_note

DEV = "cuda:0"
PATTERN = 0x7FC12345        # a quiet NaN that no arithmetic produces
GUARD = 64                  # words on each side of a destination (256 bytes: the slice keeps the allocation's alignment)


def _rnd(*shape, seed):
  return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


class Guarded(object):
  """numel floats at ``off`` floats past a 256-byte boundary, inside a buffer filled with PATTERN"""

  def __init__(self, numel, off=0):
    self.buf = torch.full((GUARD + off + numel + GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    self.lo, self.hi = GUARD + off, GUARD + off + numel
    self.view = self.buf.view(torch.float32)[self.lo:self.hi]
    assert self.view.data_ptr() % 16 == (4 * off) % 16

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


def _offset_copy(t, off):
  """t's values on the device, ``off`` floats past an aligned base -> (view, owner)"""
  owner = torch.zeros(t.numel() + off + 4, device=DEV)
  view = owner[off:off + t.numel()]
  view.copy_(t.reshape(-1))
  return view, owner


def _fwd(src, H, W, gain, dst_off=0, src_off=0, what="forward"):
  B, h, w = src.shape
  sv, owner = _offset_copy(src, src_off)
  dst = Guarded(B * H * W, dst_off)
  nat.call("as_upsample_bilinear_fwd", nat.ptr(sv), B, h, w, nat.ptr(dst.view), H, W, gain, nat.stream())
  return dst.result(what).view(B, H, W)


def _bwd(g, h, w, gain, dst_off=0, what="backward"):
  B, H, W = g.shape
  gv, owner = _offset_copy(g, 0)
  out = Guarded(B * h * w, dst_off)
  nat.call("as_upsample_bilinear_bwd", nat.ptr(gv), B, H, W, nat.ptr(out.view), h, w, gain, nat.stream())
  return out.result(what).view(B, h, w)


def _judge_fwd(src, H, W, gain, **kw):
  got = _fwd(src, H, W, gain, **kw)
  ref, bound, _ = rr.forward(src, H, W, gain)
  return rr.worst_ratio(got, ref, bound), got


def _judge_bwd(g, h, w, gain, **kw):
  got = _bwd(g, h, w, gain, **kw)
  ref, bound, _ = rr.adjoint(g, h, w, gain)
  return rr.worst_ratio(got, ref, bound), got


def _id(s):
  return "%dx%d_to_%dx%d" % tuple(s[:4])


# ============================================================================================================== forward
@pytest.mark.parametrize("shape", rr.PRODUCTION, ids=_id)
def test_forward_production(shape):
  """dense random sources; B * H is not a multiple of UP_ROWS = 4 where H allows it (540 = 4 * 135 does not), so a workgroup
  straddles two images"""
  h, w, H, W, gain = shape
  B = {375: 2, 540: 1, 75: 3}[H]
  r, _ = _judge_fwd(_rnd(B, h, w, seed=11), H, W, gain)
  parity_note("resample_fwd_production_" + _id(shape), worst_over_bound=r, B=B)
  assert r <= 1.0


@pytest.mark.parametrize("shape", rr.PYRAMID_NO_LDS + rr.PYRAMID_LDS + rr.TEMPLATE_SWITCH, ids=_id)
def test_forward_pyramid_and_template_switch(shape):
  """down-sampling with gain 1 / 2^s: source rows of 1242 run upsample_fwd_kernel<false>, rows of 960 the LDS flavour; w = 1024
  and 1025 on the same destination straddle the switch"""
  h, w, H, W, gain = shape
  B = 3 if H % 4 else 2
  r, _ = _judge_fwd(_rnd(B, h, w, seed=12), H, W, gain)
  parity_note("resample_fwd_pyramid_" + _id(shape), worst_over_bound=r, B=B, lds=int(w <= 1024))
  assert r <= 1.0


def test_forward_short_rows_and_misaligned_bases():
  """W in 1 .. 9 (pieces shorter than a vector) and W % 4 in all residues with odd H, each with the destination 0 .. 3 floats and
  the source 0 .. 1 float past an aligned base"""
  worst = 0.0
  for shape in rr.NARROW + rr.RESIDUES:
    h, w, H, W, gain = shape
    src = _rnd(2, h, w, seed=13 + W)
    for dst_off in range(4):
      for src_off in range(2):
        what = "%s dst+%d src+%d" % (_id(shape), dst_off, src_off)
        r, _ = _judge_fwd(src, H, W, gain, dst_off=dst_off, src_off=src_off, what=what)
        assert r <= 1.0, (what, r)
        worst = max(worst, r)
  parity_note("resample_fwd_short_rows_misaligned", worst_over_bound=worst, cases=len(rr.NARROW + rr.RESIDUES) * 8)


@pytest.mark.parametrize("dst_off", [0, 1, 2, 3])
def test_forward_second_pass_of_a_row(dst_off):
  """W = 4100: 1024 threads (the cap) of four pixels cover 4096, the rest takes a second pass of the X0 loop"""
  h, w, H, W, gain = rr.WIDE[0]
  r, _ = _judge_fwd(_rnd(2, h, w, seed=14), H, W, gain, dst_off=dst_off)
  parity_note("resample_fwd_second_pass_off%d" % dst_off, worst_over_bound=r)
  assert r <= 1.0


@pytest.mark.parametrize("h,w", [(7, 9), (33, 130), (5, 1030)])
def test_forward_identity_is_bit_exact(h, w):
  src = _rnd(3, h, w, seed=15)
  got = _fwd(src, h, w, 1.0, dst_off=1)
  assert torch.equal(got, src)


@pytest.mark.parametrize("h,w,H,W", [(1, 1, 5, 7), (1, 5, 3, 20), (1, 1030, 3, 1100)])
def test_forward_single_source_row_across_images(h, w, H, W):
  """h = 1: every fine row of every image reads source row 0, so only the image index tells the staged rows of one image from
  those of the next; B = 3 with H % 4 != 0 puts two images into one workgroup"""
  gain = W / w
  r, _ = _judge_fwd(_rnd(3, h, w, seed=16), H, W, gain)
  parity_note("resample_fwd_h1_%dx%d_to_%dx%d" % (h, w, H, W), worst_over_bound=r)
  assert r <= 1.0


def test_forward_constant_and_corner_sources():
  h, w, H, W, gain = rr.PRODUCTION[2]
  c = 0.7310585786300049
  src = torch.full((2, h, w), c)
  r, got = _judge_fwd(src, H, W, gain)
  exact = float(src[0, 0, 0]) * float(torch.tensor(gain, dtype=torch.float32))
  assert r <= 1.0
  assert float((got.double() - exact).abs().max()) <= 2 * 2.0 ** -23 * abs(exact), "constant source: more than 2 ulp"
  corners = torch.zeros(4, h, w)
  for b, (y, x) in enumerate([(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]):
    corners[b, y, x] = 1.0 + 0.1 * b
  rc, gotc = _judge_fwd(corners, H, W, gain)      # the bound is 0 wherever the corner does not reach: exact zeros there
  parity_note("resample_fwd_constant_corners", constant_over_bound=r, corners_over_bound=rc)
  assert rc <= 1.0
  assert float(gotc[0, 0, 0]) != 0 and float(gotc[3, H - 1, W - 1]) != 0


# ============================================================================================================= backward
@pytest.mark.parametrize("shape", rr.PRODUCTION, ids=_id)
def test_backward_production_dense_and_ones(shape):
  """dense random G, and G = 1 (all terms positive: the bound is ~K U relative, so a dropped tap of any weight above that
  shows); two launches on the same input give the same bits (a gather, no atomics)"""
  h, w, H, W, gain = shape
  B = 2
  g = _rnd(B, H, W, seed=21)
  r, got = _judge_bwd(g, h, w, gain)
  again = _bwd(g, h, w, gain)
  assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two launches differ"
  r1, _ = _judge_bwd(torch.ones(1, H, W), h, w, gain, dst_off=1)
  K, ny, nx = rr.k_bwd(h, w, H, W)
  parity_note("resample_bwd_production_" + _id(shape), dense_over_bound=r, ones_over_bound=r1, K=K, ny=ny, nx=nx)
  assert r <= 1.0 and r1 <= 1.0


def _support_ends(n, N, coarse):
  """first and last fine index with a non-zero weight on each of the coarse indices, from the reference's W"""
  Wm, _ = rr.matrices(n, N)
  out = []
  for i in coarse:
    nz = torch.nonzero(Wm[:, i]).flatten()
    out += [int(nz[0]), int(nz[-1])]
  return sorted(set(out))


@pytest.mark.parametrize("shape,rows,cols", [(rr.PRODUCTION[0], (0, 11, 23), (0, 12, 13, 77)),
                                             (rr.PRODUCTION[2], (0, 1, 5, 9), (0, 1, 8, 16)),
                                             (rr.PRODUCTION[3], (0, 46), (0, 28, 29, 144, 145, 155))],
                         ids=lambda v: _id(v) if isinstance(v, tuple) and len(v) == 5 else None)
def test_backward_impulses_on_the_support_ends(shape, rows, cols):
  """one non-zero fine pixel per image, on the first and last fine index that the reference's W gives coarse rows / columns
  (among them the columns on both sides of a chunk boundary) and at the four corners: with one term, mag is that term and the
  bound a few ulp of one weight product; a coarse pixel the impulse does not reach has bound 0 and must be exactly 0"""
  h, w, H, W, gain = shape
  Ys, Xs = _support_ends(h, H, rows), _support_ends(w, W, cols)
  at = sorted(set([(y, x) for y in Ys for x in Xs] + [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]))
  g = torch.zeros(len(at), H, W)
  for b, (y, x) in enumerate(at):
    g[b, y, x] = 1.0 + 0.37 * (b % 5)
  r, got = _judge_bwd(g, h, w, gain)
  parity_note("resample_bwd_impulses_" + _id(shape), worst_over_bound=r, impulses=len(at))
  assert r <= 1.0


def _H_with_ny(h, target):
  """a fine height whose largest row footprint (footprint() in float32) has exactly ``target`` rows"""
  for H in range(target // 2, 4 * target):
    lo, hi = rr.footprint32(h, H)
    if int((hi - lo + 1).max()) == target:
      return H
  raise AssertionError("no height with %d footprint rows" % target)


SPECIAL = rr.TALL + rr.CHUNK_ONE + rr.DOWN_ADJOINT + rr.ONE + [(3, 2, 5, 9, 4.5), (5, 7, 9, 35, 5.0)]


@pytest.mark.parametrize("shape", SPECIAL, ids=_id)
def test_backward_special_paths(shape):
  """(2, 3) <- (600, 40): 452 footprint rows, no row-weight table; W / w = 200 and 333: chunk == 1; (375, 1242) <- (47, 156): the
  adjoint of a down-sampling (chunk clamped to w, H < h); small ones"""
  h, w, H, W, gain = shape
  r, _ = _judge_bwd(_rnd(2, H, W, seed=22), h, w, gain)
  r1, _ = _judge_bwd(torch.ones(2, H, W), h, w, gain, dst_off=3)
  K, ny, nx = rr.k_bwd(h, w, H, W)
  parity_note("resample_bwd_special_" + _id(shape), dense_over_bound=r, ones_over_bound=r1, K=K, ny=ny, nx=nx)
  assert r <= 1.0 and r1 <= 1.0


@pytest.mark.parametrize("ny", [255, 256, 257])
def test_backward_around_the_row_table_limit(ny):
  """footprints of exactly 255, 256 (the last with the table) and 257 rows (the first without)"""
  h, w, W = 3, 4, 37
  H = _H_with_ny(h, ny)
  gain = W / w
  r, _ = _judge_bwd(_rnd(2, H, W, seed=23), h, w, gain)
  r1, _ = _judge_bwd(torch.ones(1, H, W), h, w, gain)
  parity_note("resample_bwd_table_limit_ny%d" % ny, dense_over_bound=r, ones_over_bound=r1, H=H)
  assert r <= 1.0 and r1 <= 1.0


def test_backward_refuses_a_ratio_beyond_the_span():
  """W / w = 400: (chunk + 2) * 400 + 6 > UPB_SPAN even at chunk == 1 -> AS_ERR_ARG, as_last_error() names the entry point, and
  nothing is launched (the pre-filled output is untouched)"""
  lib = nat.load()
  g = torch.ones(1, 1, 400, device=DEV)
  out = Guarded(1)
  rc = lib.as_upsample_bilinear_bwd(nat.ptr(g), 1, 1, 400, nat.ptr(out.view), 1, 1, 400.0, nat.stream())
  torch.cuda.synchronize()
  assert rc == -1
  msg = lib.as_last_error().decode()
  assert "as_upsample_bilinear_bwd" in msg and "scale factor" in msg, msg
  assert out.untouched()
  # the largest ratio the check admits still runs (339 fine columns per coarse column)
  r, _ = _judge_bwd(_rnd(1, 2, 339, seed=24), 1, 1, 339.0)
  assert r <= 1.0
