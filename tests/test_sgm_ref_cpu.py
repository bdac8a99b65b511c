"""tests/sgm_ref.py, the numpy restatement the GPU tests hold csrc/sgm.hip to, pinned without a GPU: against a second, deliberately
naive aggregation that follows each path geometrically from its entry pixel, against cases worked by hand, against a planted
scene it has to recover, and against six plausible mistakes (sgm_ref.WRONG), each of which a named case tells from the contract.
Then the host side: the entry points are declared and bound, and every refusal comes before the first HIP call."""
import json
import os

import numpy as np
import pytest

import sgm_ref as sg

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sgm_recovery.json")


# ------------------------------------------------------------------------------------------------- an independent aggregation
def naive_aggregate(cl, cr, D, P1, P2, paths):
  """Plain loops, one path at a time: every pixel whose predecessor lies outside the image starts a line, which is followed
  pixel by pixel until it leaves the image.  No wrap, no vectors, Python integers."""
  B, H, W = cl.shape
  S = np.zeros((B, H, W, D), dtype=np.int64)

  def cost(b, y, x, d):
    return bin(int(cl[b, y, x]) ^ int(cr[b, y, x - d])).count("1") if x - d >= 0 else 64

  for b in range(B):
    for dy, dx in sg.DIRECTIONS[paths]:
      for y in range(H):
        for x in range(W):
          if 0 <= y - dy < H and 0 <= x - dx < W:
            continue                                                    # not an entry pixel of this direction
          prev, cy, cx = None, y, x
          while 0 <= cy < H and 0 <= cx < W:
            c = [cost(b, cy, cx, d) for d in range(D)]
            if prev is None:
              cur = c
            else:
              m = min(prev)
              cur = []
              for d in range(D):
                terms = [prev[d], m + P2]
                if d > 0:
                  terms.append(prev[d - 1] + P1)
                if d < D - 1:
                  terms.append(prev[d + 1] + P1)
                cur.append(c[d] + min(terms) - m)
            for d in range(D):
              S[b, cy, cx, d] += cur[d]
            prev, cy, cx = cur, cy + dy, cx + dx
  return S


def random_census(shape, seed):
  rng = np.random.default_rng(seed)
  words = rng.integers(0, 1 << 62, size=(2,) + shape, dtype=np.int64).astype(np.uint64)
  return words[0], words[1]


@pytest.mark.parametrize("paths", (4, 8))
@pytest.mark.parametrize("shape_d", [((1, 5, 7), 4), ((2, 7, 5), 6), ((1, 1, 9), 3), ((1, 9, 1), 3), ((1, 1, 1), 1)],
                         ids=lambda s: "x".join(map(str, s[0])) + "_D%d" % s[1])
def test_aggregation_equals_a_naive_one(shape_d, paths):
  shape, D = shape_d
  cl, cr = random_census(shape, seed=sum(shape) + D)
  for P1, P2 in sg.PENALTIES:
    got = sg.aggregate(cl, cr, D, P1, P2, paths)
    want = naive_aggregate(cl, cr, D, P1, P2, paths)
    assert got.dtype == np.uint16 and np.array_equal(got.astype(np.int64), want), (P1, P2)
    assert got.max() <= paths * (64 + P2)


def test_images_through_census_equal_the_naive_aggregation():
  """the same comparison from images, W < D in part (7 x 5, D = 6)"""
  left, right = sg.random_pair(1, 3, 7, 5, shift=1, seed=4)
  cl, cr = sg.census(left), sg.census(right)
  for paths in (4, 8):
    assert np.array_equal(sg.aggregate(cl, cr, 6, 10, 120, paths).astype(np.int64), naive_aggregate(cl, cr, 6, 10, 120, paths))


# ------------------------------------------------------------------------------------------------- by hand
def test_constant_image():
  """every census word 0, every cost 0 in view and 64 out of it: d* = 0 everywhere, nothing rejected (s1 = 0: no value is below it)"""
  img = np.full((1, 3, 6, 11), 0.37, dtype=F)
  c = sg.census(img)
  assert not c.any()
  S = sg.aggregate(c, c, 5, 10, 120, 8)
  out = sg.select(S, 5, np.nan)
  assert (S[..., 0] == 0).all()
  for k in ("disp_l", "disp_r"):
    assert np.array_equal(out[k].view(np.uint32), np.zeros_like(out[k]).view(np.uint32)), k
  assert not out["code_l"].any() and not out["code_r"].any()
  assert out["counts"].tolist() == [[[66, 0, 0, 0, 0, 0, 0, 0]] * 2]


def test_one_row_shifted_by_two_by_hand():
  """One row of census words with x + 1 low bits set, so that popcount(w[a] ^ w[b]) = |a - b|; the right row is the left one
  shifted by 2.  Then C(x, d) = |d - 2| where x - d >= 0 and 64 elsewhere, and with P1 = 3, P2 = 5 the path (0, +1) is, by hand:"""
  W, D = 8, 4
  cl = np.array([[[(1 << (x + 1)) - 1 for x in range(W)]]], dtype=np.uint64)
  cr = np.zeros_like(cl)
  cr[0, 0, :W - 2] = cl[0, 0, 2:]
  C = sg.matching_cost(cl, cr, D)
  assert C[0, 0, :4].tolist() == [[2, 64, 64, 64], [2, 1, 64, 64], [2, 1, 0, 64], [2, 1, 0, 1]]
  assert C[0, 0, 4].tolist() == C[0, 0, 5].tolist() == [2, 1, 0, 1]
  L = sg.path_costs(C, 0, 1, 3, 5)
  # x = 1: m = 2, m + P2 = 7: d0 min(2, 67, 7) = 2 -> 2; d1 min(64, 5, 67, 7) = 5 -> 1 + 5 - 2; d2, d3: 7 -> 64 + 7 - 2
  # x = 2: m = 2: d1 min(4, 5, 72, 7) = 4 -> 3; d2 min(69, 7, 72, 7) = 7 -> 5; d3 min(69, 72, 7) -> 69
  # x = 3: m = 2: d1 min(3, 5, 8, 7) -> 2; d2 min(5, 6, 72, 7) -> 3; d3 min(69, 8, 7) = 7 -> 1 + 7 - 2
  # x = 4: m = 2: d1 min(2, 5, 6, 7) -> 1; d2 min(3, 5, 9, 7) -> 1; d3 min(6, 6, 7) -> 5
  # x = 5: m = 1, m + P2 = 6: d0 min(2, 4, 6) -> 2 + 2 - 1; d1 min(1, ..) -> 1; d2 min(1, ..) -> 0; d3 min(5, 4, 6) = 4 -> 1 + 4 - 1
  assert L[0, 0, :6].tolist() == [[2, 64, 64, 64], [2, 4, 69, 69], [2, 3, 5, 69], [2, 2, 3, 6], [2, 1, 1, 5], [3, 1, 0, 4]]
  out = sg.select(sg.aggregate(cl, cr, D, 3, 5, 4), 0, np.nan)
  assert np.rint(out["disp_l"][0, 0, 0, 3:6]).tolist() == [2.0] * 3 and not out["code_l"][0, 0, 0, 2:6].any()      # the shift comes back


def _select_column(s, uniqueness=0, x=None, W=None, wrong=None):
  """the left view's result at a pixel whose column is s (placed at x = len(s) unless given, so that it is in view)"""
  D = len(s)
  W = W or 2 * D + 2
  x = D if x is None else x
  S = np.full((1, 1, W, D), 1000, dtype=np.uint16)
  S[0, 0, x] = s
  out = sg.select(S, uniqueness, -1.0, wrong)
  return float(out["disp_l"][0, 0, 0, x]), int(out["code_l"][0, 0, 0, x])


def test_first_minimum_wins():
  """s = [5, 3, 3, 9]: d* = 1; den = 2 * (5 + 3 - 6) = 4, offset (5 - 3) / 4: the rule's own value and no more"""
  assert _select_column([5, 3, 3, 9]) == (1.5, 0)
  # (the last minimum, d* = 2, has the mirrored parabola and the same 1.5: minima that are not neighbours tell the two apart)
  assert _select_column([5, 3, 4, 3, 9]) == (float(F(1.0) + F(1.0) / F(6.0)), 0)
  assert _select_column([5, 3, 4, 3, 9], wrong="last_minimum") == (float(F(3.0) + F(-5.0) / F(14.0)), 0)


def test_uniqueness_at_equality_and_either_side():
  """uniqueness 5, s1 = 95: a far value v is rejected iff v * 95 < 9500, i.e. v < 100"""
  assert _select_column([200, 95, 200, 100, 200], 5) == (1.0, 0)          # equality: kept
  assert _select_column([200, 95, 200, 99, 200], 5) == (-1.0, 7)
  assert _select_column([200, 95, 200, 101, 200], 5) == (1.0, 0)
  assert _select_column([200, 95, 99, 200, 200], 5)[1] == 0               # a neighbour of the winner is not tested
  assert _select_column([99, 200, 95, 200, 200], 5)[1] == 7
  assert _select_column([200, 95, 200, 95, 200], 0)[1] == 0               # uniqueness 0 rejects nothing, equal minima included
  assert _select_column([200, 95, 200, 100, 200], 5, wrong="uniqueness_le")[1] == 7


def test_sub_pixel_edges():
  """the parabola through the winner and its two neighbours, in integers up to one fp32 division; none at either end of the
  column.  den == 0 needs s[d*-1] + s[d*+1] == 2 * s1, and a FIRST minimum has s[d*-1] > s1 and s[d*+1] >= s1: it cannot occur
  (nor den < 0), so the nearest case is the plateau to the right of the winner."""
  assert _select_column([3, 3, 3, 3]) == (0.0, 0)                         # d* = 0
  assert _select_column([3, 5, 7, 9]) == (0.0, 0)
  assert _select_column([9, 7, 5, 3]) == (3.0, 0)                         # d* = D - 1
  assert _select_column([9, 4, 4, 4, 9]) == (1.5, 0)                      # the plateau: d* = 1, den = 2 * (9 + 4 - 8) = 10, (9 - 4) / 10
  assert _select_column([10, 3, 4]) == (1.375, 0)                         # den = 2 * (10 + 4 - 6) = 16, (10 - 4) / 16
  assert _select_column([4, 3, 10]) == (0.625, 0)
  assert _select_column([10, 3, 5]) == (float(F(1.0) + F(5.0) / F(18.0)), 0)          # one correctly rounded division, one sum
  assert _select_column([10, 3, 3]) == (float(F(1.0) + F(7.0) / F(14.0)), 0)
  d, v, _ = sg.pick(np.array([[5, 4, 3]], dtype=np.int32), np.array([2]), 0)          # the column ends at n = 2: entry 2 is absent
  assert (int(d[0]), float(v[0])) == (1, 1.0)
  d, v, _ = sg.pick(np.array([[5, 3, 4, 0]], dtype=np.int32), np.array([3]), 0)       # n = 3: d* = 1 is interior, entry 3 is absent
  assert (int(d[0]), float(v[0])) == (1, float(F(1.0) + F(1.0) / F(6.0)))


def test_out_of_view_takes_precedence_over_not_unique():
  assert _select_column([200, 200, 200, 95], 5, x=2) == (-1.0, 3)         # d* = 3 > x = 2
  assert _select_column([95, 200, 200, 95], 5, x=0)[1] == 7               # d* = 0 is in view; the equal value at 3 rejects it
  assert _select_column([96, 200, 200, 95], 5, x=2) == (-1.0, 3)          # both hold: 3 wins
  assert _select_column([96, 200, 200, 95], 5, x=3) == (-1.0, 7)


def test_right_view_reads_the_diagonal_and_its_columns_shorten():
  """t[d] = S(y, x + d, d) for d < min(D, W - x): at the last D - 1 pixels of a row the column is shorter, and what lies beyond
  it neither wins nor makes the winner ambiguous"""
  W, D = 7, 4
  S = np.full((1, 1, W, D), 500, dtype=np.uint16)
  S[0, 0, 3, 2] = 7                                                       # the right view's pixel 1 sees it at d = 2
  S[0, 0, 6, 3] = 1                                                       # ... and pixel 3 at d = 3
  S[0, 0, 6, 1] = 2                                                       # ... and pixel 5 at d = 1, the end of its column (n = 2)
  S[0, 0, 6, 0] = 300                                                     # pixel 6: n = 1
  out = sg.select(S, 5, np.nan)
  dr, cr = out["disp_r"][0, 0, 0], out["code_r"][0, 0, 0]
  assert dr[1] == 2.0 and cr[1] == 0
  assert dr[3] == 3.0 and cr[3] == 0                                      # d* = n - 1: no offset
  assert dr[5] == 1.0 and cr[5] == 0
  assert dr[6] == 0.0 and cr[6] == 0
  assert cr[4] == 7 and cr[0] == 7 and cr[2] == 7 and np.isnan(dr[4])     # all 500: an equal value that is not 0 is within 5 per cent
  assert not sg.select(S, 0, np.nan)["code_r"].any()                      # uniqueness 0 rejects nothing
  assert (cr != 3).all()                                                  # the right view has no out-of-view code
  lens = np.minimum(D, W - np.arange(W))
  assert lens.tolist() == [4, 4, 4, 4, 3, 2, 1]


def test_grey_values_at_the_level_edges_and_bad_inputs():
  for k in (0, 1, 7, 128, 254, 255):
    v = F(k) / F(255.0)
    for g in (np.nextafter(v, F(-1.0)), v, np.nextafter(v, F(2.0))):
      img = np.full((1, 1, 1, 1), g, dtype=F)
      want = int(np.floor(np.clip(F(F(g) * F(255.0)) + F(0.5), 0, 255)))  # one product, one sum, in fp32
      assert sg.quantise(img)[0, 0, 0] == want and abs(want - k) <= 0
  # exactly between two levels: the sum rounds in fp32 before the floor
  half = F(0.5) / F(255.0)
  assert sg.quantise(np.full((1, 1, 1, 1), half, dtype=F))[0, 0, 0] == int(np.floor(F(half * F(255.0)) + F(0.5)))
  bad = np.array([np.nan, -0.25, 1.5, np.inf, -np.inf, -0.0], dtype=F).reshape(1, 1, 1, 6)
  assert sg.quantise(bad)[0, 0].tolist() == [0, 0, 255, 255, 0, 0]
  rgb = np.stack([np.full((1, 4), 0.2, F), np.full((1, 4), 0.5, F), np.full((1, 4), 0.9, F)])[None]
  g = (F(0.299) * F(0.2) + F(0.587) * F(0.5)) + F(0.114) * F(0.9)
  assert sg.quantise(rgb)[0, 0, 0] == int(np.floor(F(F(g) * F(255.0)) + F(0.5)))
  nanrgb = rgb.copy()
  nanrgb[0, 1, 0, 2] = np.nan
  assert sg.quantise(nanrgb)[0, 0].tolist()[2] == 0


def test_census_bits_by_hand():
  """3 x 4, smaller than the window: coordinates clamp.  The centre bit 31 and bit 63 stay 0."""
  q = np.array([[10, 20, 30, 40], [50, 60, 70, 80], [90, 100, 110, 120]], dtype=F) / F(255.0)
  c = sg.census(q[None, None])
  assert not (c >> np.uint64(63)).any() and not ((c >> np.uint64(31)) & np.uint64(1)).any()
  # the largest value sees every other one below it: all bits whose clamped neighbour is not the pixel itself
  y, x, want = 2, 3, 0
  for dy in range(-3, 4):
    for dx in range(-4, 5):
      yy, xx = min(max(y + dy, 0), 2), min(max(x + dx, 0), 3)
      if (yy, xx) != (y, x):
        want |= 1 << ((dy + 3) * 9 + dx + 4)
  assert int(c[0, y, x]) == want
  assert int(c[0, 0, 0]) == 0                                             # the smallest value: nothing below it
  # pixel (1, 1) = 60 sees 10 .. 50 below it: row 0 entirely (dy < 0), and (1, 0) for dx < 0 at dy = 0
  want = 0
  for dy in range(-3, 4):
    for dx in range(-4, 5):
      yy, xx = min(max(1 + dy, 0), 2), min(max(1 + dx, 0), 3)
      if q[yy, xx] < q[1, 1]:
        want |= 1 << ((dy + 3) * 9 + dx + 4)
  assert int(c[0, 1, 1]) == want and bin(want).count("1") == 3 * 9 + 4


# ------------------------------------------------------------------------------------------------- recovery
def recovery_rates():
  rates = {}
  r = sg.RECOVERY
  for paths in (4, 8):
    for seed in (1, 2, 3):
      left, right, d_true, scored = sg.recovery_scene(seed)
      out, _ = sg.sgm(left, right, r["D"], r["P1"], r["P2"], paths, r["uniqueness"])
      assert not (out["code_l"][0, 0][scored] == 3).any()
      rates["paths%d_seed%d" % (paths, seed)] = sg.recovery_rate(out["disp_l"], d_true, scored)
  return rates


def test_recovery_of_a_planted_scene():
  """24 x 64, D = 16: background 3, a rectangle at 12 in front of it, independent grey levels.  At least 0.90 of the left view's
  in-view, unoccluded pixels within 1 px of the truth, for 4 and 8 paths on three seeds; the six values are recorded."""
  rates = recovery_rates()
  print("recovery rates:", rates)
  recorded = json.load(open(GOLDEN))
  assert set(recorded["rates"]) == set(rates)
  for name, value in rates.items():
    assert value >= 0.90, (name, value)
    assert value == recorded["rates"][name], (name, value, recorded["rates"][name])


def test_recovery_scene_is_what_it_says():
  left, right, d_true, scored = sg.recovery_scene(1)
  assert left.shape == right.shape == (1, 1, 24, 64) and left.dtype == F
  assert (d_true[6:18, 24:44] == 12).all() and (d_true == 12).sum() == 12 * 20 and ((d_true == 3) | (d_true == 12)).all()
  ql, qr = sg.quantise(left)[0], sg.quantise(right)[0]
  y, x = np.nonzero(scored)
  assert np.array_equal(qr[y, x - d_true[y, x]], ql[y, x])                 # every scored pixel is seen by the right view where it should be
  assert not scored[:, :3].any() and not scored[6:18, 15:24].any() and scored[6:18, 24:44].all() and scored[0, 3:].all()
  assert len(np.unique(ql)) > 200


# ------------------------------------------------------------------------------------------------- wrong restatements
def test_wrong_restatements_are_caught():
  left, right = sg.random_pair(1, 1, 12, 5, shift=1, seed=8)               # H > W: the diagonals wrap
  cl, cr = sg.census(left), sg.census(right)
  right_S = sg.aggregate(cl, cr, 4, 10, 120, 8)
  differs = lambda wrong, paths=8: not np.array_equal(sg.aggregate(cl, cr, 4, 10, 120, paths, wrong=wrong).astype(np.int64),
                                                     naive_aggregate(cl, cr, 4, 10, 120, paths))
  assert np.array_equal(right_S.astype(np.int64), naive_aggregate(cl, cr, 4, 10, 120, 8))
  caught = {
    "p1_from_current": differs("p1_from_current"),
    "m_not_subtracted": differs("m_not_subtracted"),
    "no_reset_at_wrap": differs("no_reset_at_wrap") and not differs("no_reset_at_wrap", paths=4),     # only the diagonals wrap
    "out_of_view_zero": differs("out_of_view_zero"),
    "last_minimum": _select_column([5, 3, 4, 3, 9], wrong="last_minimum") != _select_column([5, 3, 4, 3, 9]),
    "uniqueness_le": _select_column([200, 95, 200, 100, 200], 5, wrong="uniqueness_le") != _select_column([200, 95, 200, 100, 200], 5),
  }
  assert set(caught) == set(sg.WRONG) and len(caught) >= 5
  assert all(caught.values()), caught


# ------------------------------------------------------------------------------------------------- the host side
def test_entry_points_are_declared_and_bound():
  from adaptive_stereo import _native as nat
  lib = nat.load()
  for name in ("as_sgm_census", "as_sgm_workspace", "as_sgm_aggregate", "as_sgm_select"):
    assert name in nat.EXPORTED_SYMBOLS and hasattr(lib, name)
  from adaptive_stereo import disp_filter, sgm
  assert sgm.CODE_NAMES == disp_filter.CODE_NAMES + ("not_unique",) and len(sgm.CODE_NAMES) == sg.CODES
  assert sgm.SGMResult._fields == ("disp_l", "disp_r", "code_l", "code_r", "counts")
  assert lib.as_sgm_workspace(4, 375, 1242, 192) == 4 * 375 * 1242 * 192 * 2
  assert lib.as_sgm_workspace(1, 1, 1, 1) == 2
  for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, -1, 1), (1, 1, 1, 0), (1, 1, 1, 257), (65536, 1, 1, 1), (1, 1 << 12, 1 << 12, 128)):
    assert lib.as_sgm_workspace(*bad) == 0, bad
  assert lib.as_sgm_workspace(1, 1 << 12, 1 << 12, 127) == (1 << 24) * 127 * 2


def test_refusals_before_any_launch():
  """every argument check returns before the first HIP call, so it runs without a GPU"""
  import ctypes
  import re
  from adaptive_stereo import _native as nat
  lib = nat.load()
  vp = ctypes.c_void_p
  p, c, q, r, s, t = vp(4096), vp(8192), vp(1 << 16), vp(1 << 17), vp(1 << 18), vp(1 << 19)    # never dereferenced
  cases = [
    ("as_sgm_census", (None, 1, 3, 1, 1, q, None), "null"),
    ("as_sgm_census", (p, 1, 3, 1, 1, None, None), "null"),
    ("as_sgm_census", (p, 0, 3, 1, 1, q, None), "shape"),
    ("as_sgm_census", (p, 1, 3, 1, -1, q, None), "shape"),
    ("as_sgm_census", (p, 1, 2, 1, 1, q, None), "C 2"),
    ("as_sgm_census", (p, 1, 4, 1, 1, q, None), "C 4"),
    ("as_sgm_census", (p, 65536, 3, 1, 1, q, None), "65535"),
    ("as_sgm_census", (p, 1, 1, 1 << 16, 1 << 15, q, None), "overflows"),
    ("as_sgm_census", (p, 1, 1, 1, 1, vp((1 << 16) + 4), None), "aligned"),
    ("as_sgm_census", (p, 1, 1, 1, 4, vp(4096 + 8), None), "alias"),                         # census inside img
    ("as_sgm_aggregate", (None, c, 1, 1, 1, 1, 10, 120, 8, q, None), "null"),
    ("as_sgm_aggregate", (p, None, 1, 1, 1, 1, 10, 120, 8, q, None), "null"),
    ("as_sgm_aggregate", (p, c, 1, 1, 1, 1, 10, 120, 8, None, None), "null"),
    ("as_sgm_aggregate", (p, c, 1, 0, 1, 1, 10, 120, 8, q, None), "shape"),
    ("as_sgm_aggregate", (p, c, 65536, 1, 1, 1, 10, 120, 8, q, None), "65535"),
    ("as_sgm_aggregate", (p, c, 1, 1, 1, 0, 10, 120, 8, q, None), "D 0"),
    ("as_sgm_aggregate", (p, c, 1, 1, 1, 257, 10, 120, 8, q, None), "D 257"),
    ("as_sgm_aggregate", (p, c, 1, 1 << 12, 1 << 12, 128, 10, 120, 8, q, None), "overflows"),
    ("as_sgm_aggregate", (p, c, 1, 1, 1, 1, 10, 120, 5, q, None), "paths 5"),
    ("as_sgm_aggregate", (p, c, 1, 1, 1, 1, 10, 120, 16, q, None), "paths 16"),
    ("as_sgm_aggregate", (p, c, 1, 1, 1, 1, -1, 120, 8, q, None), "P1 -1"),
    ("as_sgm_aggregate", (p, c, 1, 1, 1, 1, 10, 9, 8, q, None), "P2 9"),
    ("as_sgm_aggregate", (p, c, 1, 1, 1, 1, 10, 256, 8, q, None), "P2 256"),
    ("as_sgm_aggregate", (vp(4100), c, 1, 1, 1, 1, 10, 120, 8, q, None), "8-byte"),
    ("as_sgm_aggregate", (p, c, 1, 1, 1, 1, 10, 120, 8, vp((1 << 16) + 8), None), "16-byte"),
    ("as_sgm_aggregate", (p, c, 1, 1, 4, 4, 10, 120, 8, vp(4096 + 16), None), "alias"),      # the volume inside census_l
    ("as_sgm_aggregate", (p, c, 1, 1, 4, 4, 10, 120, 8, vp(8192 - 16), None), "alias"),      # ... running into census_r
    ("as_sgm_select", (None, 1, 1, 1, 1, 5, 0.0, q, None, None, None, None, None), "null"),
    ("as_sgm_select", (p, 1, 1, 0, 1, 5, 0.0, q, None, None, None, None, None), "shape"),
    ("as_sgm_select", (p, 65536, 1, 1, 1, 5, 0.0, q, None, None, None, None, None), "65535"),
    ("as_sgm_select", (p, 1, 1, 1, 300, 5, 0.0, q, None, None, None, None, None), "D 300"),
    ("as_sgm_select", (p, 1, 1 << 12, 1 << 12, 128, 5, 0.0, q, None, None, None, None, None), "overflows"),
    ("as_sgm_select", (p, 1, 1, 1, 1, -1, 0.0, q, None, None, None, None, None), "uniqueness -1"),
    ("as_sgm_select", (p, 1, 1, 1, 1, 100, 0.0, q, None, None, None, None, None), "uniqueness 100"),
    ("as_sgm_select", (p, 1, 1, 1, 1, 5, 0.0, None, None, None, None, None, None), "no output"),
    ("as_sgm_select", (vp(4096 + 8), 1, 1, 1, 1, 5, 0.0, q, None, None, None, None, None), "16-byte"),
    ("as_sgm_select", (p, 1, 1, 1, 1, 5, 0.0, vp((1 << 16) + 2), None, None, None, None, None), "4-byte"),
    ("as_sgm_select", (p, 1, 1, 4, 4, 5, 0.0, vp(4096 + 16), None, None, None, None, None), "alias"),   # disp_l inside the volume
    ("as_sgm_select", (p, 1, 1, 4, 4, 5, 0.0, q, vp((1 << 16) + 15), None, None, None, None), "alias"),  # code_l inside disp_l
    ("as_sgm_select", (p, 1, 1, 4, 4, 5, 0.0, q, r, q, None, None, None), "alias"),                      # disp_r on disp_l
    ("as_sgm_select", (p, 1, 1, 4, 4, 5, 0.0, q, r, s, r, None, None), "alias"),                         # code_r on code_l
    ("as_sgm_select", (p, 1, 1, 4, 4, 5, 0.0, q, r, s, t, vp((1 << 18) + 12), None), "alias"),           # counts inside disp_r
    ("as_sgm_select", (p, 1, 1, 4, 4, 5, 0.0, None, None, None, t, vp((1 << 19) - 60), None), "alias"),  # counts running into code_r
  ]
  for name, args, word in cases:
    assert getattr(lib, name)(*args) == -1, (name, args)
    assert re.search(word, lib.as_last_error().decode()), (name, word, lib.as_last_error())


def test_python_side_refuses_without_a_gpu_path():
  from adaptive_stereo import sgm
  with pytest.raises(RuntimeError, match="no CPU path"):
    sgm.SemiGlobalMatcher(4, 4, device="cpu")
  with pytest.raises(RuntimeError, match="no CPU path"):
    sgm.ProxyLabeler(4, 4, device="cpu")
  for kwargs, word in ((dict(maxdisp=0), "maxdisp"), (dict(maxdisp=257), "maxdisp"), (dict(maxdisp=7.5), "maxdisp"),
                       (dict(p1=-1), "p1"), (dict(p1=10, p2=9), "p2"), (dict(p2=256), "p2"), (dict(paths=6), "paths"),
                       (dict(uniqueness=100), "uniqueness"), (dict(uniqueness=-1), "uniqueness"), (dict(channels=2), "channels")):
    with pytest.raises(ValueError, match=word):
      sgm.SemiGlobalMatcher(4, 4, **kwargs)
  with pytest.raises(ValueError, match="size 0"):
    sgm.SemiGlobalMatcher(0, 4)
  with pytest.raises(ValueError, match="2\\^31"):
    sgm.SemiGlobalMatcher(1 << 12, 1 << 12, maxdisp=128)
  with pytest.raises(ValueError, match="65535"):
    sgm.SemiGlobalMatcher(1, 1, batch=65536, maxdisp=1)
  assert "NOT tuned" in sgm.SemiGlobalMatcher.__doc__


def test_sgm_baseline_takes_the_dataset_flags_of_evaluate_model():
  import evaluate_model as E
  import sgm_baseline as SB
  args = ["--dataset_path", "/data", "--dataset_name", "KittiStereo2015", "--split", "tiny", "--subsplit", "train", "--height", "64",
          "--width", "96", "--batch_size", "2", "--num_workers", "0"]
  a, b = SB.make_parser().parse_args(args), E.make_parser().parse_args(["--mode", "eval"] + args)
  for name in ("dataset_path", "dataset_name", "split", "subsplit", "scales", "batch_size", "height", "width", "splits_path", "num_workers"):
    assert getattr(a, name) == getattr(b, name), name
  assert (a.maxdisp, a.p1, a.p2, a.paths, a.uniqueness, a.proxy) == (192, 10, 120, 8, 5, False)
  assert SB.make_parser().parse_args(args + ["--proxy", "--paths", "4"]).proxy
