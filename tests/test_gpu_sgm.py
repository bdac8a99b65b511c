"""csrc/sgm.hip (as_sgm_census, as_sgm_aggregate, as_sgm_select) and adaptive_stereo.sgm on the GPU, bit for bit against
tests/sgm_ref.py (pinned on the CPU by tests/test_sgm_ref_cpu.py).  Everything is integer up to one correctly rounded fp32
division, so every comparison is exact.  Every output is written between sentinel guards, as tests/test_gpu_disp_filter.py does.

The kernels hold a pixel's D disparities four to a lane over G = 1 .. 64 lanes (G the smallest power of two with 4 G >= D), with
an 8-byte access per lane when D % 4 == 0 and 2-byte ones otherwise; the census works on tiles of 8 rows x 32 columns.  The shapes
below take every G, both access widths, W < D, one row, one column, and more than one tile, line group and workgroup."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import disp_filter_ref as df
import lr_consistency_ref as lr
import sgm_ref as sg
from dataset_fixture import make_tree
from test_gpu_disp_filter import Guarded, dev, same_bits
from adaptive_stereo import _native as nat
from adaptive_stereo import sgm as sgm_mod

DEV = "cuda:0"
F = np.float32
SENT_F, SENT_U8, SENT_I16, SENT_I32, SENT_I64 = -7777.0, 0xA5, -21555, -7777, -7777
CENSUS_SHAPES = [(1, 1), (1, 9), (9, 1), (3, 4), (7, 9), (8, 10), (9, 63), (9, 64), (9, 65), (17, 70)]
VOLUME_SHAPES = [(1, 1, 1), (1, 70, 5), (9, 1, 3), (5, 7, 16), (12, 40, 64), (40, 12, 8), (8, 65, 65), (6, 130, 192), (4, 70, 256)]
SELECT_OUTS = ("disp_l", "code_l", "disp_r", "code_r", "counts")


def as_u64(t):
  return t.cpu().numpy().view(np.uint64)


def as_u16(t):
  return t.cpu().numpy().view(np.uint16)


# ================================================================================================= as_sgm_census
def run_census(img):
  """as_sgm_census on a device image [B,C,H,W] -> uint64 numpy [B,H,W]; the output sits between guards"""
  B, C, H, W = img.shape
  g = Guarded(B * H * W, torch.int64, SENT_I64)
  nat.call("as_sgm_census", nat.ptr(img), B, C, H, W, nat.ptr(g.view), nat.stream())
  torch.cuda.synchronize()
  assert g.guards_intact(), "a write outside census"
  return as_u64(g.view).reshape(B, H, W)


@pytest.mark.parametrize("C", (1, 3))
@pytest.mark.parametrize("shape", CENSUS_SHAPES, ids=lambda s: "%dx%d" % s)
def test_census_bit_for_bit(shape, C):
  H, W = shape
  img = sg.random_images(1, C, H, W, seed=H * 100 + W + C)
  want = sg.census(img)
  d_img = dev(img)
  assert np.array_equal(run_census(d_img), want)
  assert same_bits(d_img, img), "the input was written"
  levels = (np.arange(H * W * C, dtype=F).reshape(1, C, H, W) % 256) / F(255.0)        # exact levels: the rounding edge of every one
  assert np.array_equal(run_census(dev(levels)), sg.census(levels))


def test_census_batch_of_two_off_a_misaligned_base():
  B, C, H, W = 2, 3, 7, 9                                              # 189 floats an image: the second one is never 16-byte aligned
  img = sg.random_images(B, C, H, W, seed=5)
  raw = torch.zeros(B * C * H * W + 1, dtype=torch.float32, device=DEV)
  view = raw[1:].view(B, C, H, W)                                      # the first one 4 bytes off as well
  view.copy_(dev(img))
  assert view.data_ptr() % 16 == 4
  assert np.array_equal(run_census(view), sg.census(img))
  one = sg.random_images(1, 1, 9, 65, seed=6)
  twice = np.concatenate([one, one])
  got = run_census(dev(twice))
  assert np.array_equal(got, sg.census(twice)) and np.array_equal(got[0], got[1])


# ================================================================================================= as_sgm_aggregate
def run_aggregate(cl, cr, D, P1, P2, paths):
  """as_sgm_aggregate on census words (uint64 numpy [B,H,W]) -> uint16 numpy [B,H,W,D]; the volume sits between guards"""
  B, H, W = cl.shape
  nbytes = nat.load().as_sgm_workspace(B, H, W, D)
  assert nbytes == B * H * W * D * 2
  g = Guarded(nbytes // 2, torch.int16, SENT_I16)
  assert g.view.data_ptr() % 16 == 0
  d_cl, d_cr = dev(cl.view(np.int64)), dev(cr.view(np.int64))
  nat.call("as_sgm_aggregate", nat.ptr(d_cl), nat.ptr(d_cr), B, H, W, D, P1, P2, paths, nat.ptr(g.view), nat.stream())
  torch.cuda.synchronize()
  assert g.guards_intact(), "a write outside the volume"
  assert np.array_equal(as_u64(d_cl), cl.reshape(as_u64(d_cl).shape)) and np.array_equal(as_u64(d_cr), cr.reshape(as_u64(d_cr).shape))
  return as_u16(g.view).reshape(B, H, W, D)


def assert_volume(got, want, what):
  if not np.array_equal(got, want):
    bad = np.argwhere(got != want)
    raise AssertionError("%s: %d of %d elements differ, first (b, y, x, d) %s: got %s, want %s"
                         % (what, len(bad), got.size, bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.fixture(scope="module")
def census_pairs():
  """the census words of a noisy shifted pair for every volume shape, computed once and left unchanged"""
  out = {}
  for H, W, D in VOLUME_SHAPES:
    left, right = sg.random_pair(1, 1, H, W, shift=min(2, W - 1), seed=H + 3 * W + D)
    out[(H, W, D)] = (sg.census(left), sg.census(right))
  return out


@pytest.mark.parametrize("paths", (4, 8))
@pytest.mark.parametrize("shape", VOLUME_SHAPES, ids=lambda s: "%dx%d_D%d" % s)
def test_volume_bit_for_bit(census_pairs, shape, paths):
  H, W, D = shape
  cl, cr = census_pairs[shape]
  for P1, P2 in sg.PENALTIES:
    want = sg.aggregate(cl, cr, D, P1, P2, paths)
    assert_volume(run_aggregate(cl, cr, D, P1, P2, paths), want, "P1 %d P2 %d" % (P1, P2))
    assert want.max() <= paths * (64 + P2)


@pytest.mark.parametrize("paths", (4, 8))
def test_volume_of_the_same_pair_twice_in_a_batch(census_pairs, paths):
  cl, cr = census_pairs[(12, 40, 64)]
  got = run_aggregate(np.concatenate([cl, cl]), np.concatenate([cr, cr]), 64, 10, 120, paths)
  assert_volume(got[:1], sg.aggregate(cl, cr, 64, 10, 120, paths), "first half")
  assert np.array_equal(got[0], got[1])
  other_l, other_r = census_pairs[(40, 12, 8)]                         # many short lines: more line groups than one workgroup holds
  big_l, big_r = np.concatenate([other_l] * 3), np.concatenate([other_r] * 3)
  assert_volume(run_aggregate(big_l, big_r, 8, 3, 3, paths), sg.aggregate(big_l, big_r, 8, 3, 3, paths), "batch 3")


@pytest.mark.parametrize("paths", (4, 8))
def test_recovery_scene_on_the_device(paths):
  """the planted scene of the CPU test through the whole matcher: the same volume, the same maps, the recorded rate"""
  import json
  import os
  r = sg.RECOVERY
  left, right, d_true, scored = sg.recovery_scene(2)
  want, want_S = sg.sgm(left, right, r["D"], r["P1"], r["P2"], paths, r["uniqueness"])
  m = sgm_mod.SemiGlobalMatcher(r["H"], r["W"], maxdisp=r["D"], p1=r["P1"], p2=r["P2"], paths=paths, uniqueness=r["uniqueness"],
                                channels=1, device=DEV)
  res = m(dev(left), dev(right))
  torch.cuda.synchronize()
  assert np.array_equal(as_u64(m.census(dev(left))), sg.census(left))
  assert_volume(as_u16(m.volume()), want_S, "recovery scene")
  for k in SELECT_OUTS:
    assert same_bits(getattr(res, k), want[k]), k
  rate = sg.recovery_rate(res.disp_l.cpu().numpy(), d_true, scored)
  recorded = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sgm_recovery.json")))["rates"]
  assert rate >= 0.90 and rate == recorded["paths%d_seed2" % paths]
  assert np.array_equal(m.fractions(), want["counts"].astype(np.float64) / (r["H"] * r["W"]))


# ================================================================================================= as_sgm_select
def planted_volume(B, H, W, D, seed):
  """a volume written by the test: random columns with one planted dip each, then, in row 0, the cases a random one never holds"""
  rng = np.random.default_rng(seed)
  S = rng.integers(300, 2552, size=(B, H, W, D), dtype=np.uint16)
  dip = rng.integers(0, D, size=(B, H, W, 1))
  for off, lo, hi in ((-1, 100, 400), (1, 100, 400), (0, 0, 250)):
    at = np.clip(dip + off, 0, D - 1)
    np.put_along_axis(S, at, rng.integers(lo, hi, size=at.shape, dtype=np.uint16), axis=-1)
  flat = np.full(D, 1000, dtype=np.uint16)
  cases = []
  if D >= 2:
    cases.append(("equal_minima_first_and_last", {0: 95, D - 1: 95}))   # different lanes when D > 4; d* = 0
    cases.append(("minimum_at_the_end", {D - 1: 7}))
    cases.append(("minimum_at_zero", {0: 7}))
  if D >= 5:
    cases.append(("equal_minima_in_two_lanes", {1: 50, D - 2: 50, 0: 60, 2: 70}))
    cases.append(("plateau", {1: 40, 2: 40, 3: 40}))
    cases.append(("uniqueness_equal", {1: 95, D - 1: 100}))
    cases.append(("uniqueness_below", {1: 95, D - 1: 99}))
    cases.append(("uniqueness_above", {1: 95, D - 1: 101}))
    cases.append(("neighbour_not_tested", {1: 95, 2: 96}))
    cases.append(("inexact_offset", {1: 3, 0: 10, 2: 5}))
  where = {}
  for i, (name, values) in enumerate(cases):
    for x in {min(i, W - 1), W - 1 - min(i, W - 1)}:                   # once near the left border (d* > x), once near the right
      col = flat.copy()
      for d, v in values.items():
        col[d] = v
      S[0, 0, x] = col
      where.setdefault(name, []).append(x)
  return S, where


def run_select(S, uniqueness, fill, which=SELECT_OUTS, buffers=None):
  """as_sgm_select on a volume uint16 numpy [B,H,W,D] -> {name: device tensor} of the requested outputs"""
  B, H, W, D = S.shape
  n = B * H * W
  vol = Guarded(S.size, torch.int16, SENT_I16)
  vol.view.copy_(dev(S.reshape(-1).view(np.int16)))
  g = buffers or dict(disp_l=Guarded(n, torch.float32, SENT_F), code_l=Guarded(n, torch.uint8, SENT_U8),
                      disp_r=Guarded(n, torch.float32, SENT_F), code_r=Guarded(n, torch.uint8, SENT_U8),
                      counts=Guarded(B * 2 * sg.CODES, torch.int32, SENT_I32))
  nat.call("as_sgm_select", nat.ptr(vol.view), B, H, W, D, uniqueness, fill,
           *([nat.ptr(g[k].view) if k in which else None for k in SELECT_OUTS] + [nat.stream()]))
  torch.cuda.synchronize()
  assert vol.guards_intact() and np.array_equal(as_u16(vol.view), S.reshape(-1)), "the volume was written"
  for k in SELECT_OUTS:
    assert g[k].guards_intact(), "a write outside %s" % k
    if k not in which and buffers is None:
      assert g[k].untouched(), "%s was not requested and was written" % k
  return {k: g[k].view.reshape((B, 2, sg.CODES) if k == "counts" else (B, 1, H, W)) for k in which}


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 9, 2), (1, 4, 21, 5), (2, 5, 40, 16), (1, 3, 70, 65), (1, 2, 300, 192),
                                   (1, 2, 24, 256)], ids=lambda s: "x".join(map(str, s)))
def test_select_on_planted_volumes(shape):
  B, H, W, D = shape
  S, where = planted_volume(B, H, W, D, seed=sum(shape))
  codes = set()
  for uniqueness, fill in ((5, float("nan")), (0, 0.0), (40, -0.0)):
    want = sg.select(S, uniqueness, fill)
    together = run_select(S, uniqueness, fill)
    for k in SELECT_OUTS:
      assert same_bits(together[k], want[k]), "%s at uniqueness %d, fill %r" % (k, uniqueness, fill)
    codes |= set(np.unique(want["code_l"]).tolist())
    if uniqueness == 5 and D >= 5:
      xs = lambda name: [x for x in where[name] if x >= 1]             # in view for d* = 1
      assert all(want["code_l"][0, 0, 0, x] == 0 for x in xs("uniqueness_equal") + xs("uniqueness_above") + xs("neighbour_not_tested"))
      assert all(want["code_l"][0, 0, 0, x] == 7 for x in xs("uniqueness_below"))
      assert all(want["disp_l"][0, 0, 0, x] == F(1.0) + F(5.0) / F(18.0) for x in xs("inexact_offset"))
  if D >= 5 and W > D:
    assert codes == {0, 3, 7}
  for k in SELECT_OUTS:                                                # each output alone: the same bits, nothing else written
    alone = run_select(S, 40, -0.0, which=(k,))
    assert torch.equal(alone[k].view(torch.uint8), together[k].view(torch.uint8)), "alone " + k


def test_select_overwrites_counts_and_outputs_of_an_earlier_call():
  a, _ = planted_volume(2, 5, 40, 16, seed=1)
  b, _ = planted_volume(2, 5, 40, 16, seed=2)
  n = 2 * 5 * 40
  g = dict(disp_l=Guarded(n, torch.float32, SENT_F), code_l=Guarded(n, torch.uint8, SENT_U8), disp_r=Guarded(n, torch.float32, SENT_F),
           code_r=Guarded(n, torch.uint8, SENT_U8), counts=Guarded(2 * 2 * sg.CODES, torch.int32, SENT_I32))
  first = {k: v.clone() for k, v in run_select(a, 5, float("nan"), buffers=g).items()}
  second = run_select(b, 5, float("nan"), buffers=g)
  want_a, want_b = sg.select(a, 5, np.nan), sg.select(b, 5, np.nan)
  assert not np.array_equal(want_a["counts"], want_b["counts"])
  for k in SELECT_OUTS:
    assert same_bits(first[k], want_a[k]) and same_bits(second[k], want_b[k]), k
  assert int(second["counts"].sum()) == 2 * n


def test_full_size_census_and_select():
  """1 x 375 x 1242, D = 192: the census of an image and the selection on a volume written by the test (the numpy aggregation
  at this size is too slow for a test)"""
  H, W, D = 375, 1242, 192
  img = sg.random_images(1, 3, H, W, seed=9)
  assert np.array_equal(run_census(dev(img)), sg.census(img))
  S, _ = planted_volume(1, H, W, D, seed=10)
  want = sg.select(S, 5, np.nan)
  got = run_select(S, 5, float("nan"))
  for k in SELECT_OUTS:
    assert same_bits(got[k], want[k]), k
  assert int(want["counts"][0, 0, 0]) > H * W // 2


# ================================================================================================= captured, refusals
def test_captured_graph_replayed_twice_on_a_second_pair():
  B, C, H, W, D = 2, 3, 12, 70, 20
  m = sgm_mod.SemiGlobalMatcher(H, W, batch=B, maxdisp=D, channels=C, device=DEV)
  l0, r0 = sg.random_pair(B, C, H, W, shift=3, seed=1)
  l1, r1 = sg.random_pair(B, C, H, W, shift=5, seed=2)
  eager = [t.clone() for t in m(dev(l1), dev(r1))] + [m.volume().clone()]
  want, want_S = sg.sgm(l1, r1, D)
  for k, t in zip(SELECT_OUTS, (eager[0], eager[2], eager[1], eager[3], eager[4])):
    assert same_bits(t, want[k]), k
  assert_volume(as_u16(eager[5]), want_S, "eager")
  static_l, static_r = dev(l0), dev(r0)
  side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    m(static_l, static_r)                                              # warm-up on the capturing stream
  torch.cuda.synchronize()
  with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
    result = m(static_l, static_r)
  static_l.copy_(dev(l1)); static_r.copy_(dev(r1))
  for turn in range(2):                                                # the call initialises the volume itself: no clear between
    graph.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(result._fields + ("volume",), tuple(result) + (m.volume(),), eager):
      assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "%s differs between replay %d and eager" % (name, turn)
  with pytest.raises(RuntimeError, match=r"\(2, 3, 12, 70\).*\(2, 3, 12, 8\)"):
    m(torch.zeros(B, C, H, 8, device=DEV), torch.zeros(B, C, H, 8, device=DEV))
  with pytest.raises(RuntimeError, match="contiguous fp32"):
    m(dev(l0).double(), dev(r0))


def test_refusals_set_the_error_and_launch_nothing():
  lib = nat.load()
  B, C, H, W, D = 1, 3, 2, 8, 4
  n = B * H * W
  img = torch.zeros(B, C, H, W, device=DEV)
  cen = Guarded(2 * n, torch.int64, SENT_I64)
  vol = Guarded(n * D, torch.int16, SENT_I16)
  g = dict(disp_l=Guarded(n, torch.float32, SENT_F), code_l=Guarded(n, torch.uint8, SENT_U8), disp_r=Guarded(n, torch.float32, SENT_F),
           code_r=Guarded(n, torch.uint8, SENT_U8), counts=Guarded(B * 2 * sg.CODES, torch.int32, SENT_I32))
  o = {k: nat.ptr(v.view) for k, v in g.items()}
  pi, pv, s = nat.ptr(img), nat.ptr(vol.view), nat.stream()
  pl, pr_ = nat.ptr(cen.view[:n]), nat.ptr(cen.view[n:])
  off = lambda t, nbytes: nat.c_vp(t.data_ptr() + nbytes)
  outs = (o["disp_l"], o["code_l"], o["disp_r"], o["code_r"], o["counts"])
  refused = [
    ("as_sgm_census", (None, B, C, H, W, pl, s), "null"),
    ("as_sgm_census", (pi, B, C, H, W, None, s), "null"),
    ("as_sgm_census", (pi, B, C, 0, W, pl, s), "shape"),
    ("as_sgm_census", (pi, B, 2, H, W, pl, s), "C 2"),
    ("as_sgm_census", (pi, 65536, C, H, W, pl, s), "65535"),
    ("as_sgm_census", (pi, B, C, H, W, off(cen.view, 4), s), "aligned"),
    ("as_sgm_census", (pi, B, C, H, W, pi, s), "alias"),
    ("as_sgm_aggregate", (None, pr_, B, H, W, D, 10, 120, 8, pv, s), "null"),
    ("as_sgm_aggregate", (pl, pr_, B, H, W, D, 10, 120, 8, None, s), "null"),
    ("as_sgm_aggregate", (pl, pr_, B, H, -W, D, 10, 120, 8, pv, s), "shape"),
    ("as_sgm_aggregate", (pl, pr_, B, H, W, 0, 10, 120, 8, pv, s), "D 0"),
    ("as_sgm_aggregate", (pl, pr_, B, H, W, 257, 10, 120, 8, pv, s), "D 257"),
    ("as_sgm_aggregate", (pl, pr_, B, 1 << 12, 1 << 12, 128, 10, 120, 8, pv, s), "overflows"),
    ("as_sgm_aggregate", (pl, pr_, B, H, W, D, 10, 120, 6, pv, s), "paths 6"),
    ("as_sgm_aggregate", (pl, pr_, B, H, W, D, -1, 120, 8, pv, s), "P1 -1"),
    ("as_sgm_aggregate", (pl, pr_, B, H, W, D, 10, 9, 8, pv, s), "P2 9"),
    ("as_sgm_aggregate", (pl, pr_, B, H, W, D, 10, 256, 8, pv, s), "P2 256"),
    ("as_sgm_aggregate", (pl, pr_, 65536, H, W, D, 10, 120, 8, pv, s), "65535"),
    ("as_sgm_aggregate", (pl, pr_, B, H, W, D, 10, 120, 8, off(vol.view, 8), s), "16-byte"),
    ("as_sgm_aggregate", (pl, pr_, B, H, W, D, 10, 120, 8, pl, s), "alias"),
    ("as_sgm_aggregate", (pl, pr_, B, H, W, D, 10, 120, 8, off(cen.view, 8 * n - 16), s), "alias"),
    ("as_sgm_select", (None, B, H, W, D, 5, 0.0) + outs + (s,), "null"),
    ("as_sgm_select", (pv, B, H, 0, D, 5, 0.0) + outs + (s,), "shape"),
    ("as_sgm_select", (pv, B, H, W, 300, 5, 0.0) + outs + (s,), "D 300"),
    ("as_sgm_select", (pv, B, H, W, D, 100, 0.0) + outs + (s,), "uniqueness 100"),
    ("as_sgm_select", (pv, B, H, W, D, -1, 0.0) + outs + (s,), "uniqueness -1"),
    ("as_sgm_select", (pv, B, H, W, D, 5, 0.0, None, None, None, None, None, s), "no output"),
    ("as_sgm_select", (off(vol.view, 8), B, H, W, D, 5, 0.0) + outs + (s,), "16-byte"),
    ("as_sgm_select", (pv, B, H, W, D, 5, 0.0, pv, o["code_l"], o["disp_r"], o["code_r"], o["counts"], s), "alias"),
    ("as_sgm_select", (pv, B, H, W, D, 5, 0.0, o["disp_l"], o["code_l"], o["disp_l"], o["code_r"], o["counts"], s), "alias"),
    ("as_sgm_select", (pv, B, H, W, D, 5, 0.0, o["disp_l"], o["code_l"], o["disp_r"], o["code_l"], o["counts"], s), "alias"),
    ("as_sgm_select", (pv, B, H, W, D, 5, 0.0, o["disp_l"], o["code_l"], o["disp_r"], o["code_r"], o["disp_r"], s), "alias"),
  ]
  for name, args, word in refused:
    assert getattr(lib, name)(*args) == -1, (name, word)
    assert re.search(word, lib.as_last_error().decode()), (name, word, lib.as_last_error())
  torch.cuda.synchronize()
  assert all(v.untouched() for v in g.values()) and cen.untouched() and vol.untouched() and not bool(img.any())


# ================================================================================================= ProxyLabeler
PB, PC, PH, PW, PD = 2, 3, 40, 96, 32
PROXY = dict(tol_abs=1.0, max_diff=1.0, max_size=20)


def proxy_pairs():
  """two pairs with a foreground band in front of a background, noise in the right view: every stage of the chain rejects some"""
  out = []
  for seed in (3, 4):
    rng = np.random.default_rng(seed)
    left = rng.random((PB, PC, PH, PW), dtype=F)
    right = np.roll(left, -4, axis=-1)
    right[:, :, 12:28] = np.roll(left, -11, axis=-1)[:, :, 12:28]
    noisy = rng.random((PB, 1, PH, PW)) < 0.08
    right = np.where(noisy, rng.random(left.shape, dtype=F), right).astype(F)
    out.append((left, right))
  return out


def proxy_reference(left, right):
  want, _ = sg.sgm(left, right, PD)
  chk = lr.lr_check(want["disp_l"], want["disp_r"], PROXY["tol_abs"], 0.0)
  spk = df.speckle(want["disp_l"], chk["code_l"], PROXY["max_diff"], PROXY["max_size"])
  labels = np.where(spk["code"] == 0, want["disp_l"], F(0.0)).astype(F)
  return labels, spk["code"], spk["counts"], want


def test_proxy_labeler_eager_and_replayed():
  (l0, r0), (l1, r1) = proxy_pairs()
  lab = sgm_mod.ProxyLabeler(PH, PW, batch=PB, maxdisp=PD, device=DEV, **PROXY)
  for left, right in ((l0, r0), (l1, r1)):
    labels, code, counts = lab(dev(left), dev(right))
    torch.cuda.synchronize()
    want_labels, want_code, want_counts, want = proxy_reference(left, right)
    assert same_bits(labels, want_labels) and same_bits(code, want_code) and same_bits(counts, want_counts)
    assert same_bits(lab.matcher.result().code_l, want["code_l"])
  assert {0, 1, 4, 6} <= set(np.unique(want_code).tolist()), "the scene exercises every stage"
  assert 7 in want["code_l"] and 4 in want_code                        # what the matcher rejects leaves the check as bad input
  assert 0 < np.count_nonzero(want_labels) < want_labels.size and not np.isnan(want_labels).any()
  eager = [t.clone() for t in (labels, code, counts)]
  assert not lab.captured()
  lab.capture(dev(l0), dev(r0))
  assert lab.captured()
  for turn in range(2):
    replayed = lab(dev(l1), dev(r1))                                   # a copy into the static inputs + one replay
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(replayed, eager)):
      assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "output %d differs between replay %d and eager" % (i, turn)
  ins = lab.inputs()
  assert same_bits(ins[0], l1) and same_bits(ins[1], r1)


def test_proxy_supervised_step_equals_a_step_on_the_same_labels():
  from test_gpu_supervised import META, build, _same, _state, B_, H_, W_
  from adaptive_stereo.training import SupervisedTrainer
  from adaptive_stereo.utils import synthetic as syn
  pairs = [tuple(t.to(DEV).contiguous() for t in syn.stereo_pair(B_, H_, W_, seed=seed, disparities=(4.0, 7.0))) for seed in (41, 42)]
  by_hand, proxy = SupervisedTrainer(*build(META), lr=5e-5), SupervisedTrainer(*build(META), lr=5e-5)
  hand_lab = sgm_mod.ProxyLabeler(H_, W_, batch=B_, maxdisp=META["maxdisp"], device=DEV)
  lab = sgm_mod.ProxyLabeler(H_, W_, batch=B_, maxdisp=META["maxdisp"], device=DEV)
  lib = nat.load()

  def valid_count(labels):
    """the count the loss divides by, from its own forward kernel"""
    n = labels.numel()
    out4 = torch.empty(4, dtype=torch.float32, device=DEV)
    ws = torch.empty(lib.as_khamis2_workspace(n), dtype=torch.float32, device=DEV)
    zero = torch.zeros_like(labels)
    nat.call("as_khamis2_fwd", nat.ptr(zero), nat.ptr(zero), nat.ptr(labels), n, nat.ptr(out4), nat.ptr(ws), nat.stream())
    return int(out4[3])

  def compare(left, right):
    labels = hand_lab(left, right)[0].clone()
    a = by_hand.step(left, right, labels)
    b = sgm_mod.proxy_supervised_step(proxy, lab, left, right)
    torch.cuda.synchronize()
    for name in ("total_loss", "khamis_robust_loss/0", "khamis_robust_loss/3"):
      assert float(a[name]) == float(b[name]), name
    _same(_state(by_hand), _state(proxy))
    nonzero = int(torch.count_nonzero(labels))
    assert 0 < nonzero < labels.numel() and valid_count(labels) == nonzero
    assert torch.equal(lab.labels_buffer(), labels)

  compare(*pairs[0])                                                   # both eager
  by_hand.capture(pairs[0][0], pairs[0][1], hand_lab(*pairs[0])[0].clone())
  proxy.capture(pairs[0][0], pairs[0][1], torch.zeros(B_, 1, H_, W_, device=DEV))
  lab.capture()
  own = lab.labels_buffer().data_ptr()
  compare(*pairs[1])                                                   # both captured: the labels land in the step's own input
  assert lab.labels_buffer().data_ptr() == proxy.graph_inputs()[2].data_ptr() != own
  compare(*pairs[0])
  assert proxy.graph_count() == 1 and lab.captured()


# ================================================================================================= sgm_baseline.py
def test_sgm_baseline_on_an_injected_dataset(tmp_path, capsys):
  import sgm_baseline as SB
  (l0, r0), (l1, r1) = proxy_pairs()
  gts = []
  for seed in (1, 2):
    rng = np.random.default_rng(seed)
    gt = np.full((PB, 1, PH, PW), 4.0, dtype=F)
    gt[:, :, 12:28] = 11.0
    gt[rng.random(gt.shape) < 0.5] = 0.0                               # sparse ground truth
    gts.append(gt)
  batches = [{"color_l/0": torch.from_numpy(l), "color_r/0": torch.from_numpy(r), "gt_disp_l/0": torch.from_numpy(g)}
             for (l, r), g in zip(((l0, r0), (l1, r1)), gts)]
  opt = SB.make_parser().parse_args(["--maxdisp", str(PD), "--proxy", "--speckle_size", str(PROXY["max_size"])])
  got = SB.evaluate_sgm(batches, opt)
  assert set(got) == {"sgm", "proxy"}

  def figures(disps, codes):
    rows, kept, labelled = [], 0, 0
    for disp, code, gt in zip(disps, codes, gts):
      mask = (gt > 0) & (code == 0)
      err = np.abs(disp.astype(np.float64) - gt)[mask]
      rows.append([err.mean()] + [float((err > t).mean()) for t in (2, 3, 4, 5)])
      kept += int(mask.sum()); labelled += int((gt > 0).sum())
    return np.mean(rows, axis=0), kept / labelled

  refs = [proxy_reference(l, r) for l, r in ((l0, r0), (l1, r1))]
  for name, disps, codes in (("sgm", [np.nan_to_num(w["disp_l"]) for _, _, _, w in refs], [w["code_l"] for _, _, _, w in refs]),
                             ("proxy", [lab for lab, _, _, _ in refs], [code for _, code, _, _ in refs])):
    rows, density = figures(disps, codes)
    g = got[name]
    assert g["density"] == density and 0.0 < density < 1.0, name
    assert np.allclose([g["EPE"], g["D1_all_2px"], g["D1_all_3px"], g["D1_all_4px"], g["D1_all_5px"]], rows, rtol=1e-5, atol=1e-7), name
  assert got["proxy"]["density"] < got["sgm"]["density"] and got["proxy"]["EPE"] <= got["sgm"]["EPE"]
  plain = SB.evaluate_sgm(batches, SB.make_parser().parse_args(["--maxdisp", str(PD)]))
  assert set(plain) == {"sgm"} and plain["sgm"] == got["sgm"]          # fill 0.0 and fill NaN score the same pixels
  # and through the command line's own path, on a dataset tree
  data, splits = make_tree(str(tmp_path), "KittiStereo2015", n=2, H0=70, W0=110, seed=3)
  capsys.readouterr()
  out = SB.main(SB.make_parser().parse_args(["--dataset_path", data, "--dataset_name", "KittiStereo2015", "--split", "tiny", "--subsplit",
                                             "train", "--splits_path", splits, "--batch_size", "2", "--height", "64", "--width", "96",
                                             "--num_workers", "0", "--maxdisp", "32", "--proxy"]))
  text = capsys.readouterr().out
  assert "semi-global matching (8 paths, P1 10, P2 120, uniqueness 5, 32 disparities):" in text and "proxy labels" in text
  assert set(out["sgm"]) == {"EPE", "D1_all_2px", "D1_all_3px", "D1_all_4px", "D1_all_5px", "density"}
  assert 0.0 <= out["proxy"]["density"] <= out["sgm"]["density"] <= 1.0
