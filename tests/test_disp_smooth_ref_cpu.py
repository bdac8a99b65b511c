"""tests/disp_smooth_ref.py, the numpy restatement of as_disp_wmedian's contract, pinned without a GPU: against an independent
per-pixel formulation (repeat every tap's value by its weight, sort, take element (Wt - 1) // 2), against cases whose answer is
known, and against each deliberate mutant of the contract; and the host side of the entry point and of adaptive_stereo.smooth:
the binding, every refusal before any launch, the weight table."""
import numpy as np
import pytest

import disp_smooth_ref as ds

F = ds.F


# ------------------------------------------------------------------------------------------------- the independent formulation
def loop_wmedian(disp, code_in, guide, lut, radius, fill, min_support):
  d = np.ascontiguousarray(disp, dtype=F)
  B, _, H, W = d.shape
  key = ds.keys(d)
  us = ds.usable(d, code_in)
  g = None if guide is None else ds.quantise(guide)
  table = None if lut is None else np.clip(np.asarray(lut, dtype=np.int64), 0, 65535)
  out_key = key.copy()
  code = np.zeros(d.shape, dtype=np.uint8)
  counts = np.zeros((B, ds.COUNTS), dtype=np.int32)
  for b in range(B):
    for y in range(H):
      for x in range(W):
        rep, n = [], 0
        for yy in range(max(0, y - radius), min(H, y + radius + 1)):
          for xx in range(max(0, x - radius), min(W, x + radius + 1)):
            if not us[b, 0, yy, xx]:
              continue
            w = 1 if g is None else int(table[int(np.abs(g[b, :, y, x] - g[b, :, yy, xx]).sum())])
            n += 1
            rep += [int(key[b, 0, yy, xx])] * w
        wt = len(rep)
        p_us = bool(us[b, 0, y, x])
        if wt > 0 and (p_us or (fill and n >= min_support)):
          out_key[b, 0, y, x] = sorted(rep)[(wt - 1) // 2]
          slot = int(out_key[b, 0, y, x] != key[b, 0, y, x]) if p_us else 2
        elif p_us:
          slot = 0
        else:
          slot = 3
          code[b, 0, y, x] = code_in[b, 0, y, x] if code_in is not None and code_in[b, 0, y, x] != 0 else 4
        counts[b, slot] += 1
  return dict(out=out_key.view(F), code=code, counts=counts)


def _same(a, b):
  return np.array_equal(ds.bits(a["out"]), ds.bits(b["out"])) and np.array_equal(a["code"], b["code"]) and \
    np.array_equal(a["counts"], b["counts"])


def _small_lut(seed):
  """weights small enough to repeat: 0 .. 6, zeros among them, and entries that need the clamp to 0"""
  rng = np.random.default_rng(seed)
  lut = rng.integers(-2, 7, size=ds.LUT_SIZE).astype(np.int32)
  lut[0] = 5
  return lut


@pytest.mark.parametrize("radius", range(1, ds.MAX_RADIUS + 1))
def test_restatement_equals_the_sorted_repetition(radius):
  shape = (2, 7, 9)
  for guided, channels in ((False, 3), (True, 3), (True, 1)):
    disp, code_in, guide, _ = ds.random_case(shape, seed=radius, channels=channels)
    guide = guide if guided else None
    lut = _small_lut(radius) if guided else None
    for fill, ms in ((False, 1), (True, 1), (True, ds.default_min_support(radius)), (True, 3)):
      for cin in (None, code_in):
        want = loop_wmedian(disp, cin, guide, lut, radius, fill, ms)
        got = ds.wmedian(disp, cin, guide, lut, radius, fill, ms)
        assert _same(got, want), (radius, guided, channels, fill, ms, cin is None)
        assert got["counts"].sum(axis=1).tolist() == [shape[1] * shape[2]] * shape[0]


def test_ties_and_signed_zeros_against_the_sorted_repetition():
  d = ds.ties_case((1, 6, 8), seed=2)
  assert (ds.bits(d) == 0x80000000).any() and (ds.bits(d) == 0).any()
  for radius in (1, 2):
    for fill in (False, True):
      assert _same(ds.wmedian(d, None, None, None, radius, fill, 2), loop_wmedian(d, None, None, None, radius, fill, 2))


# ------------------------------------------------------------------------------------------------- hand cases
def test_a_constant_map_is_a_fixed_point():
  d = np.full((2, 1, 9, 11), F(7.25), dtype=F)
  g = np.random.default_rng(0).random((2, 3, 9, 11)).astype(F)
  for radius in (1, 4, 7):
    r = ds.wmedian(d, None, None, None, radius)
    assert np.array_equal(ds.bits(r["out"]), ds.bits(d)) and not r["code"].any() and r["counts"].tolist() == [[99, 0, 0, 0]] * 2
    r = ds.wmedian(d, None, g, ds.weight_table(0.1, 3), radius)
    assert np.array_equal(ds.bits(r["out"]), ds.bits(d))


def test_a_single_outlier_vanishes_at_radius_1():
  d = np.full((1, 1, 7, 7), F(5), dtype=F)
  d[0, 0, 3, 3] = F(90)
  r = ds.wmedian(d, None, None, None, 1)
  assert (r["out"] == F(5)).all() and r["counts"].tolist() == [[48, 1, 0, 0]]


def test_even_count_takes_the_lower_median():
  d = np.array([[[[1.0, 2.0, 3.0, 4.0]]]], dtype=F)                  # the windows at radius 1: {1,2} {1,2,3} {2,3,4} {3,4}
  assert ds.wmedian(d, None, None, None, 1)["out"].reshape(-1).tolist() == [1.0, 2.0, 3.0, 3.0]
  assert ds.wmedian(d, None, None, None, 1, wrong="upper_median")["out"].reshape(-1).tolist() == [2.0, 2.0, 3.0, 4.0]


def test_a_step_on_a_guide_edge_stays_sharp_and_the_plain_median_rounds_its_corner():
  disp, guide, fg = ds.step_scene()
  plain = ds.wmedian(disp, None, None, None, 2)["out"]
  assert plain[0, 0, 5, 5] == F(4) and fg[5, 5], "the plain median takes the corner pixel to the background"
  sharp = ds.wmedian(disp, None, guide, ds.weight_table(0.02, 1), 2)["out"]
  assert np.array_equal(ds.bits(sharp), ds.bits(disp))
  noisy = disp.copy()
  noisy[0, 0, 7, 8] = F(1)                                           # an outlier inside the foreground still goes
  cleaned = ds.wmedian(noisy, None, guide, ds.weight_table(0.02, 1), 2)["out"]
  assert np.array_equal(ds.bits(cleaned), ds.bits(disp))


def test_an_image_smaller_than_the_window():
  d = np.array([[[[3.0, np.nan, 9.0], [1.0, 5.0, np.inf]]]], dtype=F)
  r = ds.wmedian(d, None, None, None, 7, fill=True, min_support=4)  # every window is the whole image: taps 1 3 5 9
  assert r["out"].reshape(-1).tolist() == [3.0] * 6 and not r["code"].any()
  assert r["counts"].tolist() == [[1, 3, 2, 0]]
  r = ds.wmedian(d, None, None, None, 7, fill=True, min_support=5)
  assert np.isnan(r["out"][0, 0, 0, 1]) and np.isposinf(r["out"][0, 0, 1, 2]) and r["code"].reshape(-1).tolist() == [0, 4, 0, 0, 0, 4]
  assert r["counts"].tolist() == [[1, 3, 0, 2]]


def test_zero_total_weight_passes_through_and_codes_pass_through():
  d = np.array([[[[2.0, 8.0, np.nan, 6.0]]]], dtype=F)
  d.view(np.uint32)[0, 0, 0, 2] = 0x7FC12345                        # a payload
  g = np.array([[[[0.0, 1.0, 0.5, 0.0]]]], dtype=F)
  lut = np.zeros(ds.LUT_SIZE, dtype=np.int32)                        # every weight 0
  r = ds.wmedian(d, None, g, lut, 1, fill=True, min_support=1)
  assert np.array_equal(ds.bits(r["out"]), ds.bits(d)) and r["code"].reshape(-1).tolist() == [0, 0, 4, 0]
  assert r["counts"].tolist() == [[3, 0, 0, 1]]
  code_in = np.array([[[[0, 9, 0, 2]]]], dtype=np.uint8)             # a code above 6 and one below
  r = ds.wmedian(d, code_in, None, None, 1)
  assert r["code"].reshape(-1).tolist() == [0, 9, 4, 2] and r["out"].reshape(-1)[[0, 1, 3]].tolist() == [2.0, 8.0, 6.0]
  assert ds.bits(r["out"])[0, 0, 0, 2] == 0x7FC12345


def test_guide_quantisation():
  v = np.array([np.nan, -3.0, 0.0, 0.5, 1.0, 7.0, 0.0019607844, 0.09803922], dtype=F).reshape(1, 1, 1, -1)
  assert ds.quantise(v).reshape(-1).tolist() == [0, 0, 0, 128, 255, 255, 0, 25]        # 127.5 -> 128 (even), 0.49999 -> 0


# ------------------------------------------------------------------------------------------------- wrong restatements
def _mutant_inputs():
  """(name, kwargs of wmedian) of the file's inputs: between them they tell every mutant from the contract"""
  disp, code_in, guide, lut = ds.random_case((2, 7, 9), seed=1)
  zeros = np.array([[[[0.0, -0.0, 0.0, -0.0, 5.0]]]], dtype=F)
  cases = [("random", dict(disp=disp, code_in=code_in, radius=1, fill=True, min_support=3)),
           ("random_guided", dict(disp=disp, code_in=code_in, guide=guide, lut=lut, radius=2, fill=True, min_support=3)),
           ("signed_zeros", dict(disp=zeros, radius=2)),
           ("even", dict(disp=np.array([[[[1.0, 2.0, 3.0, 4.0]]]], dtype=F), radius=1))]
  lone = np.full((1, 1, 5, 9), np.nan, dtype=F)                      # single usable pixels: their neighbours see n = 1, Wt = 1024
  lone[0, 0, 2, 2], lone[0, 0, 2, 6] = F(3), F(8)
  cases.append(("lone_guided", dict(disp=lone, guide=np.full((1, 1, 5, 9), F(0.5)), lut=ds.weight_table(0.1, 1), radius=1, fill=True,
                                    min_support=2)))
  return cases


@pytest.mark.parametrize("name", ds.WRONG)
def test_every_mutant_differs_from_the_restatement(name):
  caught = []
  for label, kw in _mutant_inputs():
    if not _same(ds.wmedian(**kw), ds.wmedian(wrong=name, **kw)):
      caught.append(label)
  assert caught, name


def test_mutant_list():
  assert set(ds.WRONG) >= {"upper_median", "unusable_taps_counted", "border_replicated", "tap_colour_as_centre", "float_order",
                           "fill_gate_on_weight"}
  with np.errstate(all="ignore"):
    for shape in ds.SHAPES:                                          # the shared random cases hold every kind of input
      d, c, g, lut = ds.random_case(shape)
      assert ds.wmedian(d, c, g, lut, 2, True, 2)["counts"].sum() == d.size
  d, c, g, lut = ds.random_case(ds.TWO_TILES_PLUS)
  assert np.isnan(d).any() and np.isposinf(d).any() and (ds.bits(d) == 0x80000000).any() and set(np.unique(c)) == set(range(8))
  assert np.isnan(g).any() and (g < 0).any() and (g > 1).any() and (lut > 65535).any() and (lut < 0).any() and (lut == 0).any()
  r = ds.wmedian(d, c, g, lut, 2, True, 2)
  assert (r["counts"] > 0).all(), "every count is exercised"


# ------------------------------------------------------------------------------------------------- the host side
def test_entry_point_is_declared_and_bound():
  import os
  from adaptive_stereo import _native as nat
  assert "as_disp_wmedian" in nat.EXPORTED_SYMBOLS and hasattr(nat.load(), "as_disp_wmedian")
  header = open(os.path.join(os.path.dirname(__file__), "..", "include", "adaptive_stereo_hip.h")).read()
  assert "int as_disp_wmedian(const float* disp, const uint8_t* code_in, const float* guide, int C, const int32_t* weight_lut" in header
  from adaptive_stereo import smooth
  assert smooth.Smoothed._fields == ("disp", "code", "counts") and len(smooth.COUNT_NAMES) == ds.COUNTS
  assert smooth.LUT_SIZE == ds.LUT_SIZE and smooth.MAX_RADIUS == ds.MAX_RADIUS
  src = open(os.path.join(os.path.dirname(smooth.__file__), "..", "csrc", "disp_smooth.hip")).read()
  assert "#define DS_SPAN %d " % ds.DS_SPAN in src and "#define DS_ROWS %d " % ds.DS_ROWS in src


def test_refusals_before_any_launch():
  """every argument check returns before the first HIP call, so it runs without a GPU"""
  import ctypes
  import re
  from adaptive_stereo import _native as nat
  lib = nat.load()
  vp = ctypes.c_void_p
  p, c, g, t, o, k = vp(4096), vp(8192), vp(1 << 14), vp(1 << 15), vp(1 << 16), vp(1 << 17)   # never dereferenced
  #        disp code_in guide C lut B  H  W  r  fill ms out code counts stream
  ok = [p, None, None, 3, None, 1, 1, 4, 1, 0, 1, o, None, None, None]
  D, CIN, G, C, T, B, H, W, R, FILL, MS, OUT, CODE, COUNTS = range(14)

  def args(**kw):
    a = list(ok)
    for name, v in kw.items():
      a[dict(D=D, CIN=CIN, G=G, C=C, T=T, B=B, H=H, W=W, R=R, FILL=FILL, MS=MS, OUT=OUT, CODE=CODE, COUNTS=COUNTS)[name]] = v
    return a

  cases = [
    (args(D=None), "null"), (args(OUT=None), "null"),
    (args(B=0), "shape"), (args(H=0), "shape"), (args(W=-4), "shape"),
    (args(H=1 << 16, W=1 << 15), "overflows"), (args(B=65536), "65535"),
    (args(G=g, T=t, C=2), "C 2"), (args(G=g, T=t, C=0), "C 0"), (args(G=g, T=t, C=4), "C 4"),
    (args(G=g), "guide"), (args(T=t), "guide"),
    (args(R=0), "radius"), (args(R=8), "radius"), (args(R=-1), "radius"),
    (args(FILL=2), "fill"), (args(FILL=-1), "fill"),
    (args(MS=0), "min_support"), (args(MS=-5), "min_support"),
    (args(D=vp(4098)), "aligned"), (args(OUT=vp((1 << 16) + 1)), "aligned"), (args(COUNTS=vp((1 << 18) + 2)), "aligned"),
    (args(G=vp((1 << 14) + 2), T=t), "aligned"), (args(G=g, T=vp((1 << 15) + 1)), "aligned"),
    (args(OUT=p), "alias"),                                          # out on disp
    (args(OUT=vp(4096 + 12)), "alias"),                              # out inside disp
    (args(CIN=c, OUT=vp(8192)), "alias"),                            # out on code_in
    (args(G=g, T=t, C=1, OUT=vp((1 << 14) + 8)), "alias"),           # out inside the guide
    (args(G=g, T=t, C=3, OUT=vp((1 << 14) + 44)), "alias"),          # ... inside its third plane
    (args(G=g, T=t, OUT=vp((1 << 15) + 3064)), "alias"),             # out inside the table
    (args(CODE=vp((1 << 16) + 15)), "alias"),                        # code inside out
    (args(CODE=vp(4096 + 3)), "alias"),                              # code inside disp
    (args(COUNTS=vp((1 << 16) + 12)), "alias"),                      # counts inside out
    (args(CODE=k, COUNTS=vp((1 << 17) - 12)), "alias"),              # code inside counts
    (args(G=g, T=t, COUNTS=vp((1 << 15) + 3068)), "alias"),          # counts on the table's last entry
  ]
  for a, word in cases:
    assert lib.as_disp_wmedian(*a) == -1, (a, word)
    assert re.search(word, lib.as_last_error().decode()), (word, lib.as_last_error())


def test_python_side_refusals():
  from adaptive_stereo import smooth
  S = smooth.DisparitySmoother
  with pytest.raises(RuntimeError, match="no CPU path"):
    S(4, 4, device="cpu")
  with pytest.raises(ValueError, match="size 0"):
    S(0, 4)
  with pytest.raises(ValueError, match="2\\^31"):
    S(1 << 16, 1 << 15)
  for bad in (0, 8, 1.5):
    with pytest.raises(ValueError, match="radius"):
      S(4, 4, radius=bad)
  with pytest.raises(ValueError, match="channels"):
    S(4, 4, channels=2)
  for bad in (0.0, -1.0, float("nan"), float("inf")):
    with pytest.raises(ValueError, match="sigma_color"):
      S(4, 4, sigma_color=bad)
  for bad in (0, -3, 2.5):
    with pytest.raises(ValueError, match="min_support"):
      S(4, 4, min_support=bad)
  for bad in (0, 9, 1.5):
    with pytest.raises(ValueError, match="iterations"):
      S(4, 4, iterations=bad)


def test_integration_points_are_off_by_default():
  import inspect
  from adaptive_stereo import disp_filter, sgm
  sig = inspect.signature(disp_filter.FilteredBothViewInference.__init__).parameters
  assert (sig["smooth_radius"].default, sig["smooth_sigma"].default, sig["smooth_fill"].default) == (0, None, False)
  assert inspect.signature(sgm.ProxyLabeler.__init__).parameters["median_radius"].default == 0
  import evaluate_model as E
  opt = E.make_parser().parse_args(["--mode", "eval"])
  assert opt.smooth_radius == 0 and opt.smooth_sigma is None and opt.smooth_fill is False
  opt = E.make_parser().parse_args(["--mode", "eval", "--smooth_radius", "3", "--smooth_sigma", "0.1", "--smooth_fill"])
  assert (opt.smooth_radius, opt.smooth_sigma, opt.smooth_fill) == (3, 0.1, True)
  import sgm_baseline as SB
  assert SB.make_parser().parse_args([]).median == 0 and SB.make_parser().parse_args(["--median", "1"]).median == 1


def test_weight_table_is_monotone_and_positive_on_its_support():
  for sigma, channels in ((0.02, 1), (0.1, 3), (5.0, 3)):
    t = ds.weight_table(sigma, channels)
    support = 255 * channels + 1
    assert t.dtype == np.int32 and t.shape == (ds.LUT_SIZE,) and t[0] == 1024
    assert (np.diff(t[:support]) <= 0).all() and (t[:support] >= 1).all() and not t[support:].any()
  assert ds.weight_table(0.02, 1)[255] == 1 and ds.weight_table(5.0, 3)[765] > 800
  # DisparitySmoother builds the same table (its construction needs the device: tests/test_gpu_disp_smooth.py compares them)
  from adaptive_stereo import smooth
  assert smooth.WEIGHT_ONE == 1024
