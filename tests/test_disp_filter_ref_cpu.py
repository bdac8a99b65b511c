"""tests/disp_filter_ref.py, the numpy restatement the GPU tests hold csrc/disp_filter.hip to, pinned without a GPU: against a
scene whose answer is known by counting, against scipy.ndimage.label where the join rule is "every usable pair", at the planted
edges of both rules by name, and against six plausible mistakes (disp_filter_ref.WRONG), each of which a shared case tells from the
contract.  Then the host side: the entry points are declared and bound, and every refusal comes before the first HIP call."""
import numpy as np
import pytest

import disp_filter_ref as df

F = np.float32


# ------------------------------------------------------------------------------------------------- the analytic scene
def test_analytic_scene_edges():
  """1 x 24 x 40: background 3.0, a 12 x 16 rectangle of 12.0, a 5 x 5 island of 7.0, one pixel of 9.0.  Every step is above
  tol 1, so the edge check flags both sides of every outline: the rectangle's 2 * 12 + 2 * 16 - 4 = 52 border pixels and the
  2 * 12 + 2 * 16 = 56 around them, the island's 16 and the 20 around them, the pixel and its 4 neighbours: 149."""
  d = df.analytic_scene()
  e = df.edge_check(d, None, 1.0, 0.0)
  flagged = e["code"][0, 0] == 5
  assert flagged.sum() == 149
  assert flagged[6:18, 10:26].sum() == 52 and not flagged[7:17, 11:25].any()
  assert e["counts"].tolist() == [[24 * 40 - 149, 0, 0, 0, 0, 149, 0]]
  assert set(np.unique(e["jump"]).tolist()) == {0.0, 4.0, 6.0, 9.0}                  # |3 - 7|, |3 - 9|, |3 - 12|; 7 and 12 never touch
  assert np.array_equal(e["valid"], (e["code"] == 0).astype(F))


def test_analytic_scene_speckles_after_edges():
  d = df.analytic_scene()
  e = df.edge_check(d, None, 1.0, 0.0)
  s = df.speckle(d, e["code"], 1.0, 9)
  assert sorted(set(s["size"][s["size"] > 0].tolist())) == [9, 140, 662]              # island 3 x 3, rectangle 10 x 14, the rest
  assert (s["code"] == 6).sum() == 9 and (s["code"] == 0).sum() == 802 and (s["code"] == 5).sum() == 149
  assert s["counts"].tolist() == [[802, 0, 0, 0, 0, 149, 9]]
  assert (df.speckle(d, e["code"], 1.0, 8)["code"] == 6).sum() == 0
  assert np.all(s["label"][e["code"] != 0] == -1) and np.all(s["size"][e["code"] != 0] == 0)
  assert s["label"][0, 0, 0, 0] == 0 and s["label"][0, 0, 23, 39] == 0                # the background is one piece, first pixel 0
  assert s["label"][0, 0, 10, 15] == 7 * 40 + 11 and s["label"][0, 0, 3, 32] == 2 * 40 + 31
  both_e, both_s = df.disparity_filter(d, None, 1.0, 0.0, 1.0, 9)
  assert np.array_equal(both_s["code"], s["code"]) and np.array_equal(both_e["jump"].view(np.uint32), e["jump"].view(np.uint32))


def test_analytic_scene_speckles_alone():
  d = df.analytic_scene()
  s = df.speckle(d, None, 1.0, 25)
  assert sorted(set(s["size"].reshape(-1).tolist())) == [1, 25, 192, 742]
  assert (s["code"] == 6).sum() == 26
  assert (df.speckle(d, None, 1.0, 24)["code"] == 6).sum() == 1
  assert (df.speckle(d, None, 1.0, 0)["code"] == 6).sum() == 0                       # max_size 0 rejects nothing
  assert s["label"][0, 0, 20, 3] == 20 * 40 + 3 and s["label"][0, 0, 6, 10] == 6 * 40 + 10


# ------------------------------------------------------------------------------------------------- against scipy
def test_every_usable_pair_joined_equals_scipy_label():
  ndimage = pytest.importorskip("scipy.ndimage")
  rng = np.random.default_rng(11)
  B, H, W = 2, 33, 70
  d = rng.uniform(0, 60, size=(B, 1, H, W)).astype(F)
  d[rng.random(d.shape) < 0.42] = np.nan
  s = df.speckle(d, None, np.inf, 5)
  components = 0
  for b in range(B):
    us = ~np.isnan(d[b, 0])
    lab, n = ndimage.label(us)                                                       # 4-connectivity is its default
    components += n
    size = np.bincount(lab.reshape(-1))[lab]
    first = ndimage.minimum(np.arange(H * W).reshape(H, W), lab, index=np.arange(n + 1))[lab]
    assert np.array_equal(s["size"][b, 0], np.where(us, size, 0))
    assert np.array_equal(s["label"][b, 0], np.where(us, first, -1))
  assert components >= 50
  assert np.array_equal(s["code"], np.where(np.isnan(d), 4, np.where(s["size"] <= 5, 6, 0)))


# ------------------------------------------------------------------------------------------------- the planted edges
def _at(out, key, where, name, dx=0):
  y, x = where[name]
  return out[key][0, 0, y, x + dx]


def test_planted_edges_of_the_edge_check():
  d, code_in, where = df.planted_case()
  e = df.edge_check(d, code_in, 1.0, 0.0)
  for name, code in (("e_below", 0), ("e_exact", 0), ("e_above", 5), ("rel_overtakes", 0), ("rel_one_sided", 5), ("neg_zero", 0)):
    assert _at(e, "code", where, name) == code and _at(e, "code", where, name, 1) == code, name      # tol_rel 0: symmetric
  assert _at(e, "jump", where, "e_exact") == F(1.0)
  assert _at(e, "jump", where, "e_below") == F(1.0) - F(2.0 ** -22)
  assert _at(e, "jump", where, "e_above") == F(1.0) + F(2.0 ** -22)
  assert _at(e, "jump", where, "neg_zero") == F(0.5)
  for name in ("nan", "inf", "negative", "neg_inf"):
    assert _at(e, "code", where, name) == 4 and _at(e, "jump", where, name).view(np.uint32) == df.QNAN_BITS, name
  # a neighbour that is not usable is skipped: neither side of the hole sees the jump across it, and has no usable neighbour
  assert [_at(e, "code", where, "hole_beside_jump", k) for k in range(3)] == [0, 4, 0]
  assert _at(e, "jump", where, "hole_beside_jump") == 0.0 and np.signbit(_at(e, "jump", where, "hole_beside_jump")) == False
  assert [_at(e, "code", where, "coded_beside_jump", k) for k in range(2)] == [0, 1]                  # the code passes through
  assert _at(e, "jump", where, "coded_beside_jump", 1).view(np.uint32) == df.QNAN_BITS
  assert e["jump"][np.isnan(d)].view(np.uint32).tolist() == [df.QNAN_BITS] * int(np.isnan(d).sum())
  # tol_rel overtakes tol_abs 0.5 at d = 16, and the tolerance is the pixel's own: one side of rel_one_sided passes
  r = df.edge_check(d, code_in, 0.5, 0.0625)
  assert _at(r, "code", where, "rel_overtakes") == 0 and _at(r, "code", where, "rel_overtakes", 1) == 0
  assert _at(r, "code", where, "rel_one_sided") == 5 and _at(r, "code", where, "rel_one_sided", 1) == 0
  assert _at(df.edge_check(d, code_in, 0.5, 0.0), "code", where, "rel_overtakes") == 5
  assert _at(r, "code", where, "e_exact") == 5
  # +inf is a tolerance, and tol_rel = inf at d = 0 is a NaN product that leaves tol_abs
  assert (df.edge_check(d, code_in, np.inf, 0.0)["code"] == 5).sum() == 0
  assert _at(df.edge_check(d, code_in, 0.25, np.inf), "code", where, "neg_zero") == 5


def test_planted_edges_of_the_speckle_pass():
  d, code_in, where = df.planted_case()
  s = df.speckle(d, code_in, 1.0, 3)
  W = d.shape[-1]
  first = lambda name: where[name][0] * W + where[name][1]
  for name, joined in (("e_below", True), ("e_exact", True), ("e_above", False), ("neg_zero", True)):
    assert _at(s, "label", where, name) == first(name) and _at(s, "size", where, name) == (2 if joined else 1), name
    assert _at(s, "label", where, name, 1) == first(name) + (0 if joined else 1), name
  for name in ("nan", "inf", "negative", "neg_inf"):
    assert _at(s, "label", where, name) == -1 and _at(s, "size", where, name) == 0 and _at(s, "code", where, name) == 4, name
  assert [_at(s, "size", where, "hole_beside_jump", k) for k in range(3)] == [1, 0, 1]
  assert [_at(s, "code", where, "coded_beside_jump", k) for k in range(2)] == [6, 1]
  assert [_at(s, "label", where, "coded_beside_jump", k) for k in range(2)] == [first("coded_beside_jump"), -1]
  # size == max_size is rejected, max_size + 1 is kept
  assert [_at(s, "code", where, "size_eq", k) for k in range(3)] == [6, 6, 6] and _at(s, "size", where, "size_eq") == 3
  assert [_at(s, "code", where, "size_plus1", k) for k in range(4)] == [0, 0, 0, 0] and _at(s, "size", where, "size_plus1", 3) == 4
  assert (df.speckle(d, code_in, 1.0, 4)["code"] == 0).sum() == 0
  assert s["counts"].sum() == d.size and s["counts"][0, 1] == 1


def test_patterns_and_boundaries_lie_where_the_kernels_have_theirs():
  shape = (1, 2 * df.DF_ROWS + 1, df.DF_SPAN + 7)
  B, H, W = shape
  s = df.speckle(df.checkerboard(shape), None, 1.0, 1)
  assert (s["size"] == 1).sum() == (H * W + 1) // 2 and (s["code"] == 6).sum() == (H * W + 1) // 2
  for name in ("comb", "serpentine", "spiral", "u_shape", "full"):
    d = df.PATTERNS[name](shape)
    s = df.speckle(d, None, 1.0, 1)
    kept = ~np.isnan(d)
    assert np.all(s["label"][kept] == 0) and np.all(s["size"][kept] == kept.sum()), name
  u = ~np.isnan(df.u_shape(shape))[0, 0]
  assert u[0, 0] and u[0, W - 1] and not u[0, 1:W - 1].any() and (W - 1) // df.DF_SPAN != 0 and H > df.DF_ROWS
  assert (~np.isnan(df.serpentine(shape))[0, 0, 1::2]).sum(axis=1).tolist() == [1] * (H // 2)
  t = df.tile_steps(shape)
  e = df.edge_check(t, None, 1.0, 0.0)
  y, x = np.indices((H, W))
  on_x = ((x % df.DF_WAVE == 0) & (x > 0)) | ((x % df.DF_WAVE == df.DF_WAVE - 1) & (x < W - 1))
  on_y = ((y % df.DF_ROWS == 0) & (y > 0)) | ((y % df.DF_ROWS == df.DF_ROWS - 1) & (y < H - 1))
  assert np.array_equal(e["code"][0, 0] == 5, on_x | on_y) and (e["code"][0, 0, df.DF_ROWS - 1:df.DF_ROWS + 1] == 5).all()
  assert any(w in (df.DF_SPAN - 1, df.DF_SPAN + 1) for _, _, w in df.SHAPES) and any(h > df.DF_ROWS for _, h, _ in df.SHAPES)


# ------------------------------------------------------------------------------------------------- wrong restatements
def _differs(a, b, keys):
  return any(not np.array_equal(a[k], b[k]) for k in keys)


def test_wrong_restatements_are_caught():
  d, code_in, _ = df.planted_case()
  scene = df.analytic_scene()
  board = df.checkerboard((1, 5, 6))
  twice = np.concatenate([df.full((1, 3, 4))] * 2)
  edge_keys, speckle_keys = ("code", "jump"), ("label", "size", "code")
  caught = {
    "eight_connected": _differs(df.speckle(board, None, 1.0, 1), df.speckle(board, None, 1.0, 1, wrong="eight_connected"), speckle_keys)
    and _differs(df.edge_check(scene), df.edge_check(scene, wrong="eight_connected"), ("code",)),
    "strict_edge": _differs(df.edge_check(d, code_in), df.edge_check(d, code_in, wrong="strict_edge"), edge_keys),
    "strict_join": _differs(df.speckle(d, code_in, 1.0, 3), df.speckle(d, code_in, 1.0, 3, wrong="strict_join"), speckle_keys),
    "tol_from_neighbour": _differs(df.edge_check(d, code_in, 0.5, 0.0625), df.edge_check(d, code_in, 0.5, 0.0625, wrong="tol_from_neighbour"),
                                   edge_keys),
    "unusable_not_skipped": _differs(df.edge_check(d, code_in), df.edge_check(d, code_in, wrong="unusable_not_skipped"), edge_keys),
    "labels_leak": _differs(df.speckle(twice, None, 1.0, 12), df.speckle(twice, None, 1.0, 12, wrong="labels_leak"), speckle_keys),
  }
  assert set(caught) == set(df.WRONG) and len(caught) >= 5
  assert all(caught.values()), caught
  # and the shared random cases tell the contract from each of them too, so the GPU comparison would
  rd, rc = df.random_case((2, 5, 63))
  assert _differs(df.edge_check(rd, rc), df.edge_check(rd, rc, wrong="strict_edge"), edge_keys)
  assert _differs(df.speckle(rd, rc), df.speckle(rd, rc, wrong="strict_join"), speckle_keys)
  same = df.speckle(twice, None, 1.0, 12)
  assert np.array_equal(same["label"][0], same["label"][1]) and (same["size"] == 12).all() and (same["code"] == 6).all()


def test_random_cases_exercise_every_code():
  codes = set()
  for shape in df.SHAPES:
    d, c = df.random_case(shape)
    e, s = df.disparity_filter(d, c, 1.0, 0.0, 1.0, 3)
    codes |= set(np.unique(s["code"]).tolist())
    assert s["counts"].sum() == d.size and e["counts"].sum() == d.size
  assert codes == set(range(df.CODES))


# ------------------------------------------------------------------------------------------------- the host side
def test_entry_points_are_declared_and_bound():
  from adaptive_stereo import _native as nat
  lib = nat.load()
  for name in ("as_disp_edge_check", "as_disp_speckle"):
    assert name in nat.EXPORTED_SYMBOLS and hasattr(lib, name)
  from adaptive_stereo import consistency, disp_filter
  assert disp_filter.CODE_NAMES == consistency.CODE_NAMES + ("discontinuity", "speckle") and len(disp_filter.CODE_NAMES) == df.CODES
  assert disp_filter.DispFilter._fields == ("code", "valid", "jump", "label", "size", "counts")


def test_refusals_before_any_launch():
  """every argument check returns before the first HIP call, so it runs without a GPU"""
  import ctypes
  import re
  from adaptive_stereo import _native as nat
  lib = nat.load()
  vp = ctypes.c_void_p
  p, c, q, r, s = vp(4096), vp(8192), vp(1 << 16), vp(1 << 17), vp(1 << 18)              # never dereferenced: every call is refused
  nan = float("nan")
  cases = [
    ("as_disp_edge_check", (None, None, 1, 1, 1, 1.0, 0.0, q, None, None, None, None), "null"),
    ("as_disp_edge_check", (p, None, 0, 1, 1, 1.0, 0.0, q, None, None, None, None), "shape"),
    ("as_disp_edge_check", (p, None, 1, 1, -2, 1.0, 0.0, q, None, None, None, None), "shape"),
    ("as_disp_edge_check", (p, None, 1, 1 << 16, 1 << 15, 1.0, 0.0, q, None, None, None, None), "overflows"),
    ("as_disp_edge_check", (p, None, 65536, 1, 1, 1.0, 0.0, q, None, None, None, None), "65535"),
    ("as_disp_edge_check", (p, None, 1, 1, 1, nan, 0.0, q, None, None, None, None), "tol_abs"),
    ("as_disp_edge_check", (p, None, 1, 1, 1, 1.0, -1.0, q, None, None, None, None), "tol_rel"),
    ("as_disp_edge_check", (p, None, 1, 1, 1, 1.0, nan, q, None, None, None, None), "tol_rel"),
    ("as_disp_edge_check", (p, None, 1, 1, 1, 1.0, 0.0, None, None, None, None, None), "no output"),
    ("as_disp_edge_check", (p, None, 1, 1, 1, 1.0, 0.0, None, None, None, vp(4098), None), "aligned"),
    ("as_disp_edge_check", (p, None, 1, 1, 4, 1.0, 0.0, vp(4096 + 15), None, None, None, None), "alias"),   # code inside disp
    ("as_disp_edge_check", (p, c, 1, 1, 4, 1.0, 0.0, c, None, None, None, None), "alias"),                  # code on code_in
    ("as_disp_edge_check", (p, None, 1, 1, 4, 1.0, 0.0, None, q, vp((1 << 16) + 12), None, None), "alias"), # jump inside valid
    ("as_disp_edge_check", (p, None, 1, 1, 4, 1.0, 0.0, None, q, None, vp((1 << 16) - 24), None), "alias"), # valid inside counts
    ("as_disp_speckle", (None, None, 1, 1, 1, 1.0, 1, q, r, None, None, None, None), "null"),
    ("as_disp_speckle", (p, None, 1, 1, 1, 1.0, 1, None, r, None, None, None, None), "null"),
    ("as_disp_speckle", (p, None, 1, 1, 1, 1.0, 1, q, None, None, None, None, None), "null"),
    ("as_disp_speckle", (p, None, 1, 0, 1, 1.0, 1, q, r, None, None, None, None), "shape"),
    ("as_disp_speckle", (p, None, 1, 1 << 15, 1 << 16, 1.0, 1, q, r, None, None, None, None), "overflows"),
    ("as_disp_speckle", (p, None, 1 << 16, 1, 1, 1.0, 1, q, r, None, None, None, None), "65535"),
    ("as_disp_speckle", (p, None, 1, 1, 1, nan, 1, q, r, None, None, None, None), "max_diff"),
    ("as_disp_speckle", (p, None, 1, 1, 1, -0.5, 1, q, r, None, None, None, None), "max_diff"),
    ("as_disp_speckle", (p, None, 1, 1, 1, 1.0, -1, q, r, None, None, None, None), "max_size"),
    ("as_disp_speckle", (p, None, 1, 1, 1, 1.0, 1, vp((1 << 16) + 2), r, None, None, None, None), "aligned"),
    ("as_disp_speckle", (p, None, 1, 1, 4, 1.0, 1, q, q, None, None, None, None), "alias"),                 # size on label
    ("as_disp_speckle", (p, None, 1, 1, 4, 1.0, 1, q, vp((1 << 16) + 12), None, None, None, None), "alias"),
    ("as_disp_speckle", (p, None, 1, 1, 4, 1.0, 1, vp(4096 + 8), r, None, None, None, None), "alias"),      # label inside disp
    ("as_disp_speckle", (p, c, 1, 1, 4, 1.0, 1, q, r, vp(8192 + 3), None, None, None), "alias"),            # code inside code_in
    ("as_disp_speckle", (p, None, 1, 1, 4, 1.0, 1, q, r, s, s, None, None), "alias"),   # valid on code
    ("as_disp_speckle", (p, None, 1, 1, 4, 1.0, 1, q, r, None, None, vp((1 << 17) + 12), None), "alias"),   # counts inside size
  ]
  for name, args, word in cases:
    assert getattr(lib, name)(*args) == -1, (name, args)
    assert re.search(word, lib.as_last_error().decode()), (name, word, lib.as_last_error())


def test_python_side_refuses_without_a_gpu_path():
  import torch
  from adaptive_stereo import disp_filter as dfm
  with pytest.raises(RuntimeError, match="no CPU path"):
    dfm.DisparityFilter(4, 4, device="cpu")
  with pytest.raises(ValueError, match="tol_abs"):
    dfm.DisparityFilter(4, 4, tol_abs=-1.0)
  with pytest.raises(ValueError, match="tol_rel"):
    dfm.DisparityFilter(4, 4, tol_rel=float("nan"))
  with pytest.raises(ValueError, match="max_diff"):
    dfm.DisparityFilter(4, 4, max_diff=float("nan"))
  with pytest.raises(ValueError, match="max_size"):
    dfm.DisparityFilter(4, 4, max_size=-1)
  with pytest.raises(ValueError, match="max_size"):
    dfm.DisparityFilter(4, 4, max_size=2.5)
  with pytest.raises(ValueError, match="size 0"):
    dfm.DisparityFilter(0, 4)
  with pytest.raises(ValueError, match="2\\^31"):
    dfm.DisparityFilter(1 << 16, 1 << 15)

  class Net(torch.nn.Module):
    pass
  scaled = Net()
  scaled.input_scale = 1
  with pytest.raises(ValueError, match="input_scale 1"):
    dfm.FilteredBothViewInference(Net(), scaled, 4, 4)
  assert issubclass(dfm.FilteredBothViewInference, dfm.consistency.BothViewInference)


def test_evaluate_model_flags_default_off():
  import evaluate_model as E
  opt = E.make_parser().parse_args(["--mode", "save"])
  assert opt.post_filter is False and opt.lr_check is False
  assert (opt.edge_tol, opt.speckle_size, opt.speckle_diff) == (1.0, 200, 1.0)
  opt = E.make_parser().parse_args(["--mode", "eval", "--post_filter", "--edge_tol", "2.5", "--speckle_size", "50", "--speckle_diff", "0.5"])
  assert opt.post_filter and (opt.edge_tol, opt.speckle_size, opt.speckle_diff) == (2.5, 50, 0.5)
