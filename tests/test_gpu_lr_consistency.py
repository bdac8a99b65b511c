"""csrc/lr_consistency.hip (as_mirror_pair, as_flip_w, as_lr_check, as_lr_fill) and adaptive_stereo.consistency.LeftRightConsistency
on the GPU, bit for bit against tests/lr_consistency_ref.py (pinned on the CPU by tests/test_lr_consistency_ref_cpu.py).  Every
output is written between sentinel guards, as tests/test_gpu_confidence.py does.

as_lr_fill covers FILL_SPAN = 1024 pixels of a row per workgroup pass (256 lanes of 4 pixels; a wave covers 256): W = 1242 takes
two passes in either direction, and lr_consistency_ref.fill_case puts invalid runs across pixel 1023|1024, across 1023|1024 counted
from the row's end, and across the wave boundaries of both directions."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lr_consistency_ref as lr
from adaptive_stereo import _native as nat
from adaptive_stereo import consistency as cons
from guarded_buffers import DEV, SENTINEL, SENTINEL_I32, SENTINEL_U8, Guarded, same_bits

FLOAT_OUTS = ("valid_l", "valid_r", "diff_l", "diff_r")
ALL_OUTS = ("code_l", "code_r") + FLOAT_OUTS + ("counts",)
SHAPE_IDS = ["x".join(map(str, s)) for s in lr.SHAPES]
FILL_SHAPES = lr.SHAPES + [(1, 10, 1242), (1, 10, 300)]             # + every pattern of fill_case at a two-pass and a one-pass width


def bits(t):
  return t.contiguous().view(torch.int32)


# ================================================================================================= as_lr_check
def run_check(L, R, tol, mirrored=0, which=ALL_OUTS):
  """as_lr_check on two device maps [B,1,H,W] -> {name: device tensor} of the requested outputs; asserts that nothing else was
  written"""
  B, _, H, W = L.shape
  n = B * H * W
  gc = Guarded(2, n, torch.uint8, SENTINEL_U8)
  gf = Guarded(4, n)
  gi = Guarded(1, B * 2 * lr.CODES, torch.int32, SENTINEL_I32)
  views = dict(zip(ALL_OUTS, gc.views + gf.views + gi.views))
  nat.call("as_lr_check", nat.ptr(L), nat.ptr(R), mirrored, B, H, W, tol[0], tol[1],
           *([nat.ptr(views[k]) if k in which else None for k in ALL_OUTS] + [nat.stream()]))
  torch.cuda.synchronize()
  assert gc.guards_intact() and gf.guards_intact() and gi.guards_intact(), "a write outside the outputs"
  for k in ALL_OUTS:
    if k not in which:
      sentinel = SENTINEL_I32 if k == "counts" else SENTINEL_U8 if k.startswith("code") else SENTINEL
      assert bool((views[k] == sentinel).all()), "%s was not requested and was written" % k
  return {k: views[k].reshape((B, 2, lr.CODES) if k == "counts" else (B, 1, H, W)) for k in which}


@pytest.fixture(scope="module")
def check_cases():
  """the inputs and the restatement's answer of every case, computed once and left unchanged"""
  out = {}
  for shape in lr.SHAPES:
    L, R, _ = lr.check_case(shape)
    for tol in lr.TOLS:
      out[(shape, tol)] = (L, R, lr.lr_check(L, R, *tol))
  return out


@pytest.mark.parametrize("tol", lr.TOLS, ids=lambda t: "tol%g_%g" % t)
@pytest.mark.parametrize("shape", lr.SHAPES, ids=SHAPE_IDS)
def test_check_bit_for_bit(check_cases, shape, tol):
  Ln, Rn, want = check_cases[(shape, tol)]
  L, R = torch.from_numpy(Ln).to(DEV), torch.from_numpy(Rn).to(DEV)
  together = run_check(L, R, tol)
  for k in ALL_OUTS:
    assert same_bits(together[k], want[k]), k
  mirrored = run_check(L, torch.from_numpy(lr.flip_w(Rn)).to(DEV), tol, mirrored=1)      # the network's layout: equal bits
  for k in ALL_OUTS:
    assert torch.equal(mirrored[k].view(torch.uint8), together[k].view(torch.uint8)), "mirrored " + k
  for k in ALL_OUTS:                                                # each output alone: the same bits, nothing else written
    alone = run_check(L, R, tol, which=(k,))
    assert torch.equal(alone[k].view(torch.uint8), together[k].view(torch.uint8)), "alone " + k


def test_counts_are_overwritten_not_accumulated(check_cases):
  shape, tol = (2, 4, 63), lr.TOLS[0]
  Ln, Rn, want = check_cases[(shape, tol)]
  lrc = cons.LeftRightConsistency(shape[1], shape[2], batch=shape[0], tol_abs=tol[0], tol_rel=tol[1], device=DEV)
  L, R = torch.from_numpy(Ln).to(DEV), torch.from_numpy(Rn).to(DEV)
  first = lrc.check(L, R)
  assert same_bits(first.counts, want["counts"])
  other_l, other_r = torch.from_numpy(lr.flip_w(Rn)).to(DEV), torch.from_numpy(lr.flip_w(Ln)).to(DEV)    # other data, same buffers
  second = lrc.check(other_l, other_r)
  want2 = lr.lr_check(lr.flip_w(Rn), lr.flip_w(Ln), *tol)
  assert not np.array_equal(want2["counts"], want["counts"])
  assert same_bits(second.counts, want2["counts"])
  for k in ALL_OUTS:
    assert same_bits(getattr(second, k), want2[k]), k
  assert np.array_equal(lrc.fractions(), want2["counts"].astype(np.float64) / (shape[1] * shape[2]))
  third = lrc.check(L, torch.from_numpy(lr.flip_w(Rn)).to(DEV), mirrored=True)                            # and the class's mirrored route
  for k in ALL_OUTS:
    assert same_bits(getattr(third, k), want[k]), k


# ================================================================================================= as_lr_fill
@pytest.mark.parametrize("shape", FILL_SHAPES, ids=["x".join(map(str, s)) for s in FILL_SHAPES])
def test_fill_bit_for_bit(shape):
  B, H, W = shape
  dn, cn = lr.fill_case(shape)
  want = lr.lr_fill(dn, cn)
  disp, code = torch.from_numpy(dn).to(DEV), torch.from_numpy(cn).to(DEV)
  g = Guarded(1, B * H * W)
  nat.call("as_lr_fill", nat.ptr(disp), nat.ptr(code), B, H, W, nat.ptr(g.views[0]), nat.stream())
  torch.cuda.synchronize()
  assert g.guards_intact(), "a write outside the output"
  got = g.views[0].reshape(B, 1, H, W)
  if not same_bits(got, want):
    bad = np.argwhere(got.cpu().numpy().view(np.uint32) != want.view(np.uint32))
    raise AssertionError("%d pixels differ, first (b, 0, y, x) = %s" % (len(bad), bad[:8].tolist()))
  assert torch.equal(disp.cpu(), torch.from_numpy(dn)), "the input was written"
  # the class: its own buffer, a caller's buffer, and the refusal of an alias
  lrc = cons.LeftRightConsistency(H, W, batch=B, device=DEV)
  assert same_bits(lrc.fill(disp, code), want)
  mine = torch.empty_like(disp)
  assert lrc.fill(disp, code, out=mine) is mine and same_bits(mine, want)
  with pytest.raises(RuntimeError, match="alias"):
    lrc.fill(disp, code, out=disp)


# ================================================================================================= as_mirror_pair, as_flip_w
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("W", [1, 3, 4, 66, 128, 1242])          # 4 and 128 take the four-element route when aligned
def test_mirror_pair_and_flip(W, C):
  B, H = 2, 3
  gen = torch.Generator().manual_seed(W * 10 + C)
  raw = torch.randn(2 * B * C * H * W + 8, generator=gen).to(DEV)
  n = B * C * H * W
  for offset in (0, 1):                                             # 1: a base pointer one float off 16-byte alignment
    left = raw[offset:offset + n].view(B, C, H, W)
    right = raw[offset + n + 4:offset + 2 * n + 4].view(B, C, H, W)
    want_l = torch.cat([left, torch.flip(right, (-1,))])
    want_r = torch.cat([right, torch.flip(left, (-1,))])
    g = Guarded(2, 2 * n)
    nat.call("as_mirror_pair", nat.ptr(left), nat.ptr(right), B, C, H, W, nat.ptr(g.views[0]), nat.ptr(g.views[1]), nat.stream())
    torch.cuda.synchronize()
    assert g.guards_intact()
    assert torch.equal(bits(g.views[0].view(2 * B, C, H, W)), bits(want_l)), (W, C, offset, "left_batch")
    assert torch.equal(bits(g.views[1].view(2 * B, C, H, W)), bits(want_r)), (W, C, offset, "right_batch")
    # misaligned outputs as well
    gm = Guarded(1, 4 * n + 6)
    lb, rb = gm.views[0][1:1 + 2 * n], gm.views[0][2 * n + 2:4 * n + 2]
    nat.call("as_mirror_pair", nat.ptr(left), nat.ptr(right), B, C, H, W, nat.ptr(lb), nat.ptr(rb), nat.stream())
    g2 = Guarded(1, n)
    nat.call("as_flip_w", nat.ptr(left), B * C, H, W, nat.ptr(g2.views[0]), nat.stream())
    torch.cuda.synchronize()
    assert gm.guards_intact() and g2.guards_intact()
    assert torch.equal(bits(lb.view(2 * B, C, H, W)), bits(want_l)) and torch.equal(bits(rb.view(2 * B, C, H, W)), bits(want_r))
    assert bool((gm.views[0][0] == SENTINEL) & (gm.views[0][2 * n + 1] == SENTINEL) & (gm.views[0][4 * n + 2:] == SENTINEL).all())
    assert torch.equal(bits(g2.views[0].view(B, C, H, W)), bits(torch.flip(left, (-1,)))), (W, C, offset, "flip_w")
  # the Python wrappers: one buffer whose halves are the two batches
  left, right = raw[:n].view(B, C, H, W).clone(), raw[n:2 * n].view(B, C, H, W).clone()
  lb, rb = cons.mirror_pair(left, right)
  assert torch.equal(bits(lb), bits(torch.cat([left, torch.flip(right, (-1,))])))
  assert torch.equal(bits(rb), bits(torch.cat([right, torch.flip(left, (-1,))])))
  assert rb.data_ptr() == lb.data_ptr() + 4 * lb.numel()
  assert torch.equal(bits(cons.flip_w(left)), bits(torch.flip(left, (-1,))))


# ================================================================================================= refusals
def test_refusals_set_the_error_and_launch_nothing():
  lib = nat.load()
  B, H, W = 1, 2, 8
  n = B * H * W
  x = torch.zeros(B, 1, H, W, device=DEV)
  code = torch.zeros(B, 1, H, W, dtype=torch.uint8, device=DEV)
  g = Guarded(4, 2 * n)
  gc = Guarded(1, n, torch.uint8, SENTINEL_U8)
  o = [nat.ptr(v) for v in g.views]
  px, pc, s = nat.ptr(x), nat.ptr(code), nat.stream()
  nothing = (None,) * 6
  refused = [
    ("as_mirror_pair", (None, px, B, 1, H, W, o[0], o[1], s), "null"),
    ("as_mirror_pair", (px, px, B, 1, H, 0, o[0], o[1], s), "shape"),
    ("as_mirror_pair", (px, px, B, 1, H, W, o[0], o[0], s), "alias"),
    ("as_mirror_pair", (o[0], o[1], B, 1, H, W, o[1], o[2], s), "alias"),       # left_batch over right
    ("as_mirror_pair", (o[0], o[1], B, 1, H, W, o[2], o[0], s), "alias"),       # right_batch over left
    ("as_mirror_pair", (o[0], o[1], B, 1, H, W, o[2], o[1], s), "alias"),       # right_batch over right
    ("as_flip_w", (px, 1, H, W, None, s), "null"),
    ("as_flip_w", (px, 0, H, W, o[0], s), "shape"),
    ("as_flip_w", (o[0], 1, H, W, o[0], s), "alias"),
    ("as_lr_check", (px, None, 0, B, H, W, 1.0, 0.0, nat.ptr(gc.views[0]), None, o[0], None, None, None, None, s), "null"),
    ("as_lr_check", (px, px, 0, B, -1, W, 1.0, 0.0, nat.ptr(gc.views[0]), None, o[0], None, None, None, None, s), "shape"),
    ("as_lr_check", (px, px, 0, B, H, (1 << 24) + 8, 1.0, 0.0, nat.ptr(gc.views[0]), None, o[0], None, None, None, None, s), "2\\^24"),
    ("as_lr_check", (px, px, 3, B, H, W, 1.0, 0.0, nat.ptr(gc.views[0]), None, o[0], None, None, None, None, s), "mirrored"),
    ("as_lr_check", (px, px, 0, B, H, W, float("inf"), 0.0, nat.ptr(gc.views[0]), None, o[0], None, None, None, None, s), "tol_abs"),
    ("as_lr_check", (px, px, 0, B, H, W, 1.0, 0.0) + nothing + (None, s), "no output"),
    ("as_lr_fill", (px, None, B, H, W, o[0], s), "null"),
    ("as_lr_fill", (px, pc, 0, H, W, o[0], s), "shape"),
    ("as_lr_fill", (o[0], pc, B, H, W, o[0], s), "alias"),
  ]
  import re
  for name, args, word in refused:
    assert getattr(lib, name)(*args) == -1, name
    assert re.search(word, lib.as_last_error().decode()), (name, word, lib.as_last_error())
  torch.cuda.synchronize()
  assert bool((g.raw == SENTINEL).all()) and bool((gc.raw == SENTINEL_U8).all())
  lrc = cons.LeftRightConsistency(H, W, batch=B, device=DEV)
  with pytest.raises(RuntimeError, match=r"\(1, 1, 2, 8\).*\(1, 1, 2, 4\)"):
    lrc.check(x, torch.zeros(B, 1, H, 4, device=DEV))
  with pytest.raises(RuntimeError, match="contiguous fp32"):
    lrc.check(x.double(), x)
  with pytest.raises(RuntimeError, match="uint8"):
    lrc.fill(x, x)
