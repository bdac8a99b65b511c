"""tests/visualization_ref.py (the numpy restatement of include/adaptive_stereo_hip.h's colour-map contract) against the
reference's own outputs in tests/golden/visualization.npz, the packaged tables against the fixture's, and the table extraction
from a colour-map object.  No GPU, no matplotlib, no cv2."""
import os
import re

import numpy as np
import pytest

import visualization_ref as R
from adaptive_stereo.utils import visualization as V
from conftest import GOLDEN_DIR, PKG

CASES = [(shape, config) for shape in R.SHAPES for config in R.configs_for(shape)]
IDS = [R.case_name(s, c) for s, c in CASES]


@pytest.fixture(scope="module")
def fixture():
  return np.load(os.path.join(GOLDEN_DIR, "visualization.npz"), allow_pickle=False)


def same(a, b):
  """Equal shapes, dtypes and bits."""
  a, b = np.asarray(a), np.asarray(b)
  return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_neither_matplotlib_nor_cv2_is_imported_by_the_package():
  pattern = re.compile(r"^\s*(import|from)\s+(matplotlib|cv2)\b", re.M)
  for root, _, files in os.walk(PKG):
    for f in files:
      if f.endswith(".py"):
        assert not pattern.search(open(os.path.join(root, f)).read()), os.path.join(root, f)


def test_packaged_tables_are_the_fixtures(fixture):
  tables = V.packaged_colormaps()
  assert sorted(tables) == sorted(R.MAPS)
  for name in R.MAPS:
    assert tables[name].shape == (259, 4) and same(tables[name], fixture["table__" + name]), name
    t = tables[name]
    # what the header's notes on the named maps rest on
    assert same(t[256], t[0]) and same(t[257], t[255]) and not t[258].any(), name
    assert same(V.table_u8(t)[:, :3], R.table_u8(t))
  table, n = V.resolve_colormap(None)
  assert n == 256 and same(table, tables["magma"])
  assert same(V.resolve_colormap(None, default="gray")[0], tables["gray"])
  with pytest.raises(ValueError, match="unknown colour map"):
    V.resolve_colormap("viridis")


@pytest.mark.parametrize("shape,config", CASES, ids=IDS)
def test_restatement_is_the_reference_bit_for_bit(fixture, shape, config):
  kind, vmin, vmax, cmap = config
  name = R.case_name(shape, config)
  x = R.make_case(shape, kind)
  assert np.array_equal(R.checksum(x), fixture["check__" + name])
  table = fixture["table__" + cmap]
  idx = R.index(x, vmin, vmax)
  assert idx.dtype == np.int16 and idx.min() >= 0 and idx.max() <= 258
  assert same(R.paint_u8(table, idx, "bgr"), fixture["u8__" + name])
  assert same(R.paint_u8(table, idx, "rgb"), fixture["u8__" + name][..., ::-1].copy())
  if R.stores_float(shape, config):
    assert same(R.paint_f32(table, idx), fixture["f32__" + name])
    assert same(R.paint_rgba(table, idx), fixture["rgba__" + name])
  else:
    assert "f32__" + name not in fixture.files


def test_planted_values_do_what_the_contract_says(fixture):
  """Read off the reference's own bytes: a NaN under fixed bounds blackens one pixel, under automatic bounds its whole image and
  no other; a constant image is black; +inf under automatic bounds leaves entry 0 everywhere else."""
  shape = R.SHAPES[2]
  magma = R.table_u8(fixture["table__magma"])[:, ::-1]                       # BGR rows
  last = shape[2] * shape[3] - 1
  u8 = fixture["u8__" + R.case_name(shape, ("nan", 0, 80, "magma"))].reshape(2, -1, 3)
  assert not u8[0, last].any() and int((u8 == 0).all(axis=2).sum()) == 1
  u8 = fixture["u8__" + R.case_name(shape, ("nan", None, None, "magma"))].reshape(2, -1, 3)
  assert not u8[0].any()
  plain = R.paint_u8(fixture["table__magma"], R.index(R.make_case(shape, "nan")[1:], None, None)).reshape(-1, 3)
  assert same(u8[1], plain), "image 1 is painted with its own range"
  u8 = fixture["u8__" + R.case_name(shape, ("constant", None, None, "magma"))]
  assert not u8.any()
  u8 = fixture["u8__" + R.case_name(shape, ("pinf", None, None, "magma"))].reshape(2, -1, 3)
  assert not u8[0, last].any() and bool((u8[0, :last] == magma[0]).all())
  u8 = fixture["u8__" + R.case_name(shape, ("infs", 0, 80, "magma"))].reshape(2, -1, 3)
  assert same(u8[0, last - 1], magma[257]) and same(u8[0, last], magma[256])  # +inf: over, -inf: under
  # (0, 80): k * 0.3125 is exactly t == k, its predecessor the last value of bin k - 1; 80 itself is N - 1, -0.0 is 0
  x = R.make_case(shape, "edges80")
  idx = R.index(x, 0, 80).reshape(2, -1)
  flat = x.reshape(2, -1)
  n = 5 + 2 * 255
  planted, got = flat[0, -n:], idx[0, -n:]
  assert got[:5].tolist() == [0, 255, 257, 256, 255] and np.signbit(planted[0])
  assert got[5::2].tolist() == list(range(1, 256)) and got[6::2].tolist() == list(range(0, 255))


def test_reciprocal_restatement_differs_on_the_planted_case(fixture):
  biters = fixture["reciprocal_biters"]
  assert len(biters) >= 1 and same(biters, R.reciprocal_biters(0, R.R115))
  for shape in R.SHAPES[1:]:
    config = ("edges115", 0, R.R115, "inferno")
    x = R.make_case(shape, "edges115")
    good, wrong = R.index(x, 0, R.R115), R.index(x, 0, R.R115, reciprocal=True)
    assert (good != wrong).any(), "the planted values do not tell a reciprocal from a division at %s" % (shape,)
    table = fixture["table__inferno"]
    assert same(R.paint_u8(table, good), fixture["u8__" + R.case_name(shape, config)])
    assert not same(R.paint_u8(table, wrong), fixture["u8__" + R.case_name(shape, config)])


def test_den_is_the_rounded_difference_of_the_python_floats():
  lo, den = R.bounds(np.zeros((1, 1), np.float32), 0.3, 77.7)
  assert den == np.float32(77.7 - 0.3) and den != np.float32(77.7) - np.float32(0.3)
  automatic, lo2, hi2, den2 = V._bounds(0.3, 77.7)
  assert automatic == 0 and np.float32(lo2) == lo and np.float32(den2) == den
  assert V._bounds(None, 5)[0] == 1 and V._bounds(0, None)[0] == 2 and V._bounds(None, None)[0] == 3


def test_conversions_restated(fixture):
  for hw in R.CONVERSION_SHAPES:
    tag = "%dx%d" % hw
    if "cv_rgb__" + tag in fixture.files:
      assert same(R.to_cv_rgb(R.make_image(3, hw)), fixture["cv_rgb__" + tag])
    assert same(R.to_cv_gray(R.make_image(1, hw)), fixture["cv_gray__" + tag])
    d = R.make_disp_image(hw)
    assert same(R.to_cv_disp(d), fixture["cv_disp__" + tag])
    assert same(R.to_cv_disp(d, cast_uint8=False), fixture["cv_disp_f32__" + tag])
    assert same(R.to_cv_disp(d), fixture["cv_disp_2d__" + tag])
  assert same(R.saturate_u8(np.array([-3.0, np.nan, 0.5, 254.9, 255.0, 1e9, np.inf], np.float32)),
              np.array([0, 0, 0, 254, 255, 255, 255], np.uint8))


TenSteps = R.TenSteps


def test_table_of_a_duck_typed_colour_map():
  table, n = V.colormap_table(TenSteps())
  assert n == 10 and table.shape == (13, 4) and table.dtype == np.float64
  assert np.array_equal(table[:10, 0], np.arange(10) / 9.0)
  assert table[10].tolist() == [1, 0, 0, 1] and table[11].tolist() == [0, 0, 1, 1] and table[12].tolist() == [0, 1, 0, 1]
  assert same(V.resolve_colormap(TenSteps())[0], table)
  x = np.array([[-1.0, 0.0, 0.5, 0.99, 1.0, 1.5, np.nan]], np.float32).reshape(1, 1, 1, 7)
  assert R.index(x, 0, 1, N=10).ravel().tolist() == [10, 0, 5, 9, 9, 11, 12]

  class TooMany(TenSteps):
    N = 257
  with pytest.raises(ValueError, match="outside"):
    V.colormap_table(TooMany())


def test_host_helpers_keep_the_reference_shapes(fixture):
  a = np.zeros((5, 7, 3))
  assert V.maybe_put_channel_dim_first(a).shape == (3, 5, 7) and V.maybe_put_channel_dim_last(a).shape == (5, 7, 3)
  assert V.maybe_put_channel_dim_last(np.zeros((1, 5, 7))).shape == (5, 7, 1)
  x = R.make_case(R.SHAPES[2], "plain")
  rgb = R.paint_rgba(fixture["table__jet"], R.index(x[:1]))[0, :, :, :3]
  assert same(V.float_image_to_cv_uint8(rgb, encoding="rgb"), fixture["float_image_rgb__37x53"])
  assert same(V.float_image_to_cv_uint8(rgb, encoding="bgr"), fixture["float_image_rgb__37x53"][..., ::-1].copy())
