"""tests/lr_consistency_ref.py, the numpy restatement the GPU tests hold csrc/lr_consistency.hip to, pinned on the CPU against a
scene whose answer is known in closed form, against the planted edge cases by name, and against the invariants of the contract.
The last tests check the host side of the feature that needs no GPU: the ABI table, the refusals, the reference's signature."""
import numpy as np
import pytest

import lr_consistency_ref as lr

F = np.float32


# ------------------------------------------------------------------------------------------------- the analytic scene
def test_analytic_scene_left_view():
  s = lr.SCENE
  L, R = lr.analytic_scene()
  out = lr.lr_check(L, R)                                           # the defaults: tol_abs 1, tol_rel 0
  code = out["code_l"][0, 0]
  band = int(s["FG"] - s["BG"])
  assert band == 9
  expect = np.zeros((s["H"], s["W"]), dtype=np.uint8)
  expect[:, :int(s["BG"])] = 3                                      # out of view exactly where x < d
  expect[s["y0"]:s["y1"], s["x0"] - band:s["x0"]] = 1               # the band left of the rectangle, occluded
  assert np.array_equal(code, expect)
  assert np.array_equal(out["valid_l"][0, 0], (expect == 0).astype(F))
  diff = out["diff_l"][0, 0]
  assert (lr.bits(diff[expect == 3]) == lr.QNAN_BITS).all()
  assert (diff[expect == 1] == F(band)).all() and (diff[expect == 0] == 0).all()


def test_analytic_scene_right_view_is_the_mirror_statement():
  s = lr.SCENE
  L, R = lr.analytic_scene()
  code = lr.lr_check(L, R)["code_r"][0, 0]
  band, fg = int(s["FG"] - s["BG"]), int(s["FG"])
  expect = np.zeros((s["H"], s["W"]), dtype=np.uint8)
  expect[:, s["W"] - int(s["BG"]):] = 3                             # x + d > W - 1
  expect[s["y0"]:s["y1"], s["x1"] - fg:s["x1"] - fg + band] = 1     # the band right of the rectangle as the right view sees it
  assert np.array_equal(code, expect)
  # and literally: the right view of (L, R) is the left view of the scene mirrored in x with the views swapped
  mirrored = lr.lr_check(lr.flip_w(R), lr.flip_w(L))
  assert np.array_equal(lr.flip_w(mirrored["code_l"]), lr.lr_check(L, R)["code_r"])


def test_fill_takes_the_background():
  s = lr.SCENE
  L, R = lr.analytic_scene()
  filled = lr.lr_fill(L, lr.lr_check(L, R)["code_l"])[0, 0]
  band = int(s["FG"] - s["BG"])
  assert (filled[s["y0"]:s["y1"], s["x0"] - band:s["x0"]] == F(s["BG"])).all()      # 3, never 12
  assert (filled[:, :int(s["BG"])] == F(s["BG"])).all()                             # the border strip: only a right neighbour
  assert np.array_equal(filled, L[0, 0])                                            # which here restores the true left map


# ------------------------------------------------------------------------------------------------- planted pixels, by name
def _planted(tol):
  shape = (2, 4, 63)
  L, R, plants = lr.check_case(shape)
  out = lr.lr_check(L, R, *tol)

  def at(name):
    view, b, y, x = plants[name]
    side = "lr"[view]
    return int(out["code_" + side][b, 0, y, x]), out["diff_" + side][b, 0, y, x]
  return at


def test_planted_edges_decide_as_the_contract_says():
  at = _planted((1.0, 0.0))
  one = F(1.0)
  assert at("d0_u0")[0] != 3 and at("d0_uW1")[0] != 3               # u exactly 0 / exactly W - 1 is in view
  assert at("u0") == (0, F(0)) and at("uW1") == (0, F(0))
  assert at("nan_neighbour") == (0, F(0))                           # t == 0: the NaN at i1 does not reach r
  assert at("e_below") == (0, np.nextafter(one, F(0)))
  assert at("e_exact") == (0, one)
  assert at("e_above_occ") == (1, np.nextafter(one, F(2)))
  assert at("e_above_mis") == (2, np.nextafter(one, F(2)))


def test_tol_rel_overtakes_tol_abs():
  assert _planted((0.5, 0.0))("rel_overtakes") == (1, F(0.75))      # outside tol_abs alone
  assert _planted((0.5, 0.05))("rel_overtakes") == (0, F(0.75))     # inside max(0.5, 0.05 * 20) = 1


def test_bad_inputs_are_code_4_and_stay_in_their_pixel():
  L, R, _ = lr.check_case((2, 3, 64))
  out = lr.lr_check(L, R)
  bad = ~(L >= 0) | np.isinf(L)
  assert bad.any() and (out["code_l"][bad] == 4).all()
  assert (lr.bits(out["diff_l"][out["code_l"] >= 3]) == lr.QNAN_BITS).all()
  assert not np.isnan(out["diff_l"][out["code_l"] < 3]).any()


# ------------------------------------------------------------------------------------------------- invariants
@pytest.mark.parametrize("shape", lr.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("tol", lr.TOLS, ids=lambda t: "tol%g_%g" % t)
def test_check_invariants(shape, tol):
  B, H, W = shape
  L, R, _ = lr.check_case(shape)
  plain = lr.lr_check(L, R, *tol)
  mirrored = lr.lr_check(L, lr.flip_w(R), *tol, mirrored=True)
  for k in plain:
    a, b = plain[k], mirrored[k]
    assert np.array_equal(lr.bits(a), lr.bits(b)) if a.dtype == F else np.array_equal(a, b), k
  assert plain["counts"].dtype == np.int32 and plain["counts"].shape == (B, 2, 5)
  assert (plain["counts"].sum(axis=2) == H * W).all()               # the codes partition the pixels
  for side in "lr":
    assert plain["code_" + side].max() <= 4
    assert np.array_equal(plain["valid_" + side], (plain["code_" + side] == 0).astype(F))
  if W >= 63:
    assert set(np.unique(plain["code_l"])) == {0, 1, 2, 3, 4}       # the cases exercise every code


@pytest.mark.parametrize("shape", lr.SHAPES + [(1, 10, 1242), (1, 10, 300)], ids=lambda s: "x".join(map(str, s)))
def test_fill_invariants(shape):
  disp, code = lr.fill_case(shape)
  out = lr.lr_fill(disp, code)
  ok = code == 0
  assert np.array_equal(lr.bits(out[ok]), lr.bits(disp[ok]))        # code 0 copies its input
  empty = ~ok.any(axis=-1, keepdims=True) & np.ones_like(ok)
  assert (lr.bits(out[empty]) == 0).all()                           # a row without code 0 is +0.0
  for d_row, c_row, o_row in zip(disp.reshape(-1, shape[2]), code.reshape(-1, shape[2]), out.reshape(-1, shape[2])):
    if (c_row == 0).any():                                          # ... and only such a row: elsewhere every value is a valid one's
      assert np.isin(lr.bits(o_row), lr.bits(d_row[c_row == 0])).all()
  # idempotent on the codes' complement: with every pixel declared valid nothing changes, and filling the filled map under the
  # same codes gives the same map
  assert np.array_equal(lr.bits(lr.lr_fill(out, np.zeros_like(code))), lr.bits(out))
  assert np.array_equal(lr.bits(lr.lr_fill(out, code)), lr.bits(out))
  # every filled value is the smaller of its two nearest valid neighbours, by a plain loop
  flat_d, flat_c, flat_o = disp.reshape(-1, shape[2]), code.reshape(-1, shape[2]), out.reshape(-1, shape[2])
  for row in range(flat_d.shape[0]):
    valid = np.flatnonzero(flat_c[row] == 0)
    for x in np.flatnonzero(flat_c[row] != 0)[::7]:
      left, right = valid[valid < x], valid[valid > x]
      cands = ([flat_d[row, left[-1]]] if left.size else []) + ([flat_d[row, right[0]]] if right.size else [])
      assert flat_o[row, x] == (min(cands) if cands else 0)


def test_fill_patterns_reach_the_boundaries():
  """the wide case puts invalid runs across the pass boundary and the wave boundaries of either scan direction"""
  W = 1242
  assert W > lr.FILL_SPAN
  disp, code = lr.fill_case((1, 10, W))
  rows = dict(zip(lr.FILL_PATTERNS, code[0, 0]))
  assert (rows["pass_boundaries"][lr.FILL_SPAN - 1:lr.FILL_SPAN + 1] != 0).all()
  assert (rows["pass_boundaries"][W - lr.FILL_SPAN - 1:W - lr.FILL_SPAN + 1] != 0).all()
  assert (rows["wave_boundaries"][lr.FILL_WAVE - 1:lr.FILL_WAVE + 1] != 0).all() and (rows["wave_boundaries"][63:65] != 0).all()
  assert (rows["all_valid"] == 0).all() and (rows["all_invalid"] != 0).all() and (rows["single_valid"] == 0).sum() == 1
  run = np.flatnonzero(rows["long_run"] != 0)
  assert run.size > lr.FILL_WAVE and (np.diff(run) == 1).all()
  assert rows["ends_invalid"][0] != 0 and rows["ends_invalid"][-1] != 0


def test_mirror_and_flip():
  rng = np.random.default_rng(3)
  a, b = rng.random((2, 3, 4, 5), dtype=F), rng.random((2, 3, 4, 5), dtype=F)
  lb, rb = lr.mirror_pair(a, b)
  assert lb.shape == (4, 3, 4, 5) and np.array_equal(lb[:2], a) and np.array_equal(lb[2:, ..., 0], b[..., 4])
  assert np.array_equal(rb[:2], b) and np.array_equal(rb[2:], a[..., ::-1])


# ------------------------------------------------------------------------------------------------- the host side
def test_entry_points_are_declared_and_bound():
  from adaptive_stereo import _native as nat
  lib = nat.load()
  for name in ("as_mirror_pair", "as_flip_w", "as_lr_check", "as_lr_fill"):
    assert name in nat.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_refusals_before_any_launch():
  """every argument check returns before the first HIP call, so it runs without a GPU"""
  import ctypes
  from adaptive_stereo import _native as nat
  lib = nat.load()
  p = ctypes.c_void_p(4096)                                         # never dereferenced: every call below is refused
  q = ctypes.c_void_p(8192)
  cases = [
    ("as_mirror_pair", (None, p, 1, 1, 1, 1, q, q, None), "null"),
    ("as_mirror_pair", (p, p, 0, 1, 1, 1, q, q, None), "shape"),
    ("as_mirror_pair", (p, p, 1, 1, 1, 1, q, q, None), "alias"),
    ("as_mirror_pair", (p, p, 1, 1, 1, 4, q, ctypes.c_void_p(8192 + 16), None), "alias"),       # unequal pointers, overlapping ranges
    ("as_mirror_pair", (p, p, 1, 1, 1, 4, ctypes.c_void_p(4096 + 8), q, None), "alias"),        # an output inside an input
    ("as_mirror_pair", (p, p, 1 << 30, 1 << 10, 1 << 10, 1 << 20, q, ctypes.c_void_p(12288), None), "exceed"),
    ("as_flip_w", (p, 1, 1, 1, None, None), "null"),
    ("as_flip_w", (p, 1, 1, 1, p, None), "alias"),
    ("as_flip_w", (p, 1, 1, 4, ctypes.c_void_p(4096 + 12), None), "alias"),
    ("as_flip_w", (p, 1, 0, 1, q, None), "shape"),
    ("as_flip_w", (p, 1 << 31, 1, 1, q, None), "shape"),
    ("as_lr_check", (p, None, 0, 1, 1, 1, 1.0, 0.0, q, None, None, None, None, None, None, None), "null"),
    ("as_lr_check", (p, p, 0, 1, 1, 0, 1.0, 0.0, q, None, None, None, None, None, None, None), "shape"),
    ("as_lr_check", (p, p, 0, 1, 1, (1 << 24) + 1, 1.0, 0.0, q, None, None, None, None, None, None, None), "2\\^24"),
    ("as_lr_check", (p, p, 0, 1, 1 << 16, 1 << 16, 1.0, 0.0, q, None, None, None, None, None, None, None), "overflows"),
    ("as_lr_check", (p, p, 2, 1, 1, 1, 1.0, 0.0, q, None, None, None, None, None, None, None), "mirrored"),
    ("as_lr_check", (p, p, 0, 1, 1, 1, float("nan"), 0.0, q, None, None, None, None, None, None, None), "tol_abs"),
    ("as_lr_check", (p, p, 0, 1, 1, 1, 1.0, -1.0, q, None, None, None, None, None, None, None), "tol_rel"),
    ("as_lr_check", (p, p, 0, 1, 1, 1, 1.0, 0.0, None, None, None, None, None, None, None, None), "no output"),
    ("as_lr_fill", (p, None, 1, 1, 1, q, None), "null"),
    ("as_lr_fill", (p, p, 1, 1, 1, p, None), "alias"),
    ("as_lr_fill", (p, q, 1, 1, 4, ctypes.c_void_p(4096 + 4), None), "alias"),
    ("as_lr_fill", (p, p, 1, 1, -3, q, None), "shape"),
    ("as_lr_fill", (p, p, 1 << 16, 1 << 16, 1, q, None), "rows"),
  ]
  import re
  for name, args, word in cases:
    assert getattr(lib, name)(*args) == -1, (name, args)
    assert re.search(word, lib.as_last_error().decode()), (name, word, lib.as_last_error())


def test_python_side_refuses_without_a_gpu_path():
  import torch
  from adaptive_stereo import consistency as cons
  with pytest.raises(RuntimeError, match="no CPU path"):
    cons.LeftRightConsistency(4, 4, device="cpu")
  with pytest.raises(ValueError, match="tol_abs"):
    cons.LeftRightConsistency(4, 4, tol_abs=-1.0)
  with pytest.raises(RuntimeError, match="no CPU path"):
    cons.flip_w(torch.zeros(1, 1, 2, 2))

  class Net(torch.nn.Module):
    pass
  scaled = Net()
  scaled.input_scale = 1
  with pytest.raises(ValueError, match="input_scale 1"):
    cons.BothViewInference(Net(), scaled, 4, 4)                     # the maps would not be [B,1,height,width]
  f, s = Net(), Net()
  with pytest.raises(RuntimeError, match="inference only"):
    cons.predict_disparity_leftright(f, s, None, None)              # training mode: refused before anything is touched


def test_adapt_module_keeps_the_reference_signature():
  import inspect
  import adapt
  from adaptive_stereo.control import State
  assert list(inspect.signature(adapt.predict_disparity_leftright).parameters) == \
      ["feature_net", "stereo_net", "left", "right", "adapt_state", "opt"]
  with pytest.raises(NotImplementedError, match="leftright_consistency"):
    adapt.predict_disparity_leftright(None, None, None, None, State.IN_PROGRESS, None)
  with pytest.raises(ValueError, match="adapt_state"):
    adapt.predict_disparity_leftright(None, None, None, None, None, None)
