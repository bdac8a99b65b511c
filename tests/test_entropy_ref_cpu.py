"""tests/entropy_ref.py (the numpy restatement of as_image_entropy's contract) against the reference's own utils/entropy.py,
through tests/golden/entropy.npz (tests/golden/make_golden_entropy.py).

The bound.  The restatement sums in fp64 and rounds once; the reference takes torch's fp32 log2 and an fp32 sum in an order it
does not pin.  How far those two lie apart on the fixture's images was measured by the generator from the reference's own
results (tests/golden/entropy_bound.json); the assertion is 2 x that figure, the margin being for torch's summation order.  The
0-, 1- and 2-bit images have p = 1, 1/2 and 1/4, where every operation is exact: those are asserted exactly.
"""
import json
import os

import numpy as np
import pytest

import entropy_ref as R
from conftest import GOLDEN_DIR

BOUND = json.load(open(os.path.join(GOLDEN_DIR, "entropy_bound.json")))


@pytest.fixture(scope="module")
def fixture():
  return np.load(os.path.join(GOLDEN_DIR, "entropy.npz"), allow_pickle=False)


def test_fixture_inputs_are_the_generators():
  z = np.load(os.path.join(GOLDEN_DIR, "entropy.npz"), allow_pickle=False)
  names = [str(n) for n in z["names"]]
  assert set(R.EXACT_BITS) <= set(names)
  assert len(names) >= 16 and any(z["img__" + n].ndim == 2 for n in names) and any(z["img__" + n].shape[0] == 3 for n in names)
  assert any(z["img__" + n].min() < 0 and z["img__" + n].max() > 1 for n in names), "no image with values outside the bins"


def test_exact_images_give_exactly_0_1_and_2_bits(fixture):
  for name, bits in R.EXACT_BITS.items():
    gray = R.scores64(fixture["img__" + name])[0]
    assert gray == bits and float(fixture["gray__" + name]) == bits, name
    sc, _ = R.batch(fixture["img__" + name][None])
    assert sc[0, 0] == np.float32(bits)


def test_restatement_agrees_with_the_reference_within_twice_the_measured_gap(fixture):
  worst = {"gray": 0.0, "grad": 0.0}
  seen = 0
  for name in (str(n) for n in fixture["names"]):
    if name in R.EXACT_BITS:
      continue
    img = fixture["img__" + name]
    want64 = dict(zip(("gray", "grad"), R.scores64(img)))
    for col in ("gray", "grad"):
      key = col + "__" + name
      if key not in fixture.files:
        continue
      gap = float(R.ulp_gap(fixture[key], np.float32(want64[col])))
      print("%s %s: reference %r restatement %r gap %.2f ulp" % (name, col, float(fixture[key]), float(want64[col]), gap))
      assert name in BOUND["per_image"][col]                  # (the per-image figures are the generator's record, not a bar)
      assert gap <= 2.0 * BOUND["worst_ulp"][col], (name, col, gap)
      worst[col] = max(worst[col], gap)
      seen += 1
  assert seen >= 20
  print("worst gap here %s, recorded by the generator %s" % (worst, BOUND["worst_ulp"]))
  assert 0.0 < BOUND["worst_ulp"]["gray"] <= 4.0 and 0.0 < BOUND["worst_ulp"]["grad"] <= 4.0    # fp32 log2 and a 256-term sum


def test_batch_is_per_image_and_normalises_by_the_plane(fixture):
  names = [str(n) for n in fixture["names"] if fixture["img__" + str(n)].ndim == 3 and fixture["img__" + str(n)].shape[0] == 3]
  img = fixture["img__" + names[0]]
  sc, hist = R.batch(np.stack([img, img[::-1].copy()]))
  assert hist[0, 0].sum() == img.size and np.array_equal(hist[0], hist[1])      # planes in another order: the same counts
  assert hist[0, 1].sum() == 3 * img.shape[1] * (img.shape[2] - 1)
  assert sc[0, 0] == np.float32(R.scores64(img)[0]) and np.array_equal(sc[0], sc[1])
  one_pixel_wide = R.batch(np.zeros((1, 1, 4, 1), np.float32))
  assert one_pixel_wide[0][0, 0] == 0.0 and np.isnan(one_pixel_wide[0][0, 1]) and one_pixel_wide[1][0, 1].sum() == 0


def test_binning_identities_against_a_plain_loop():
  """All 256 intensities and all 511 differences, through counts() and against loops that know no formula."""
  f = np.float32
  pixel = []                                   # pixel[v]: the smallest fp32 x with (int)(255.0f * x) == v
  for v in range(256):
    x = f(v) / f(255.0)
    while int(f(255.0) * x) < v:
      x = np.nextafter(x, f(2.0))
    assert int(f(255.0) * x) == v
    pixel.append(x)
    count_g, count_d = R.counts(np.array([[x]], np.float32))
    want = np.zeros(256, np.int64); want[v] = 1
    assert np.array_equal(count_g, want) and count_d.sum() == 0 and R.gray_bin(v) == v
  for v in (-1, 256, 300, -255):
    assert R.gray_bin(v) == -1
  seen = np.zeros(256, np.int64)
  for d in range(-255, 256):
    q = 0                                      # the plain loop: the last of 256 equal bins over [-255, 255] that starts at or below d
    while q < 255 and (q + 1) * 510 <= (d + 255) * 256:
      q += 1
    assert R.grad_bin(d) == q, d
    a = 0 if d >= 0 else 255
    _, count_d = R.counts(np.array([[pixel[a], pixel[a + d]]], np.float32))
    want = np.zeros(256, np.int64); want[q] = 1
    assert np.array_equal(count_d, want), d
    seen[q] += 1
  assert seen.sum() == 511 and seen.min() == 1 and seen.max() == 2
  for d in (-256, 256, 1000):
    assert R.grad_bin(d) == -1


def test_invalid_pixels_and_range_edges():
  f = np.float32
  x = np.array([[f("nan"), 0.5, f("inf"), 0.5, f(1e10), 0.5, f("-inf"), 0.5, 0.5]], np.float32)
  count_g, count_d = R.counts(x)
  assert count_g.sum() == 5 and count_g[127] == 5
  assert count_d.sum() == 1 and count_d[R.grad_bin(0)] == 1            # only the last pair has two valid pixels
  v, ok = R.quantise(np.array([-0.001, -1 / 255.0, 1.0, np.nextafter(f(1.0), f(2.0)), 256 / 255.0, 8421504.0, 8421505.0], np.float32))
  # 255 * 8421504 = 2147483520 is the largest fp32 below 2^31; 255 * 8421505 rounds to 2^31 itself
  assert v.tolist()[:6] == [0, -1, 255, 255, 256, 2147483520] and ok.tolist() == [True] * 6 + [False]
  pair = np.array([[300 / 255.0 + 1e-4, 100 / 255.0 + 1e-4]], np.float32)           # v = 300 has no bin; d = -200 has
  count_g, count_d = R.counts(pair)
  assert count_g.sum() == 1 and count_g[100] == 1 and count_d[R.grad_bin(-200)] == 1
