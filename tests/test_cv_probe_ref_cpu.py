"""tests/cv_probe_ref.py — the host restatement that tests/test_gpu_cv_probe.py compares csrc/cv_probe.hip against — held to things
that do not depend on it: the reference's own picks and values (tests/golden/cv_probe.npz), exact fp64 arithmetic, a pixel worked
by hand; the argument checks of as_cost_volume_probe, which return before any launch and need no GPU; the sorting network of
csrc/sort_net.h on the host; and the pure half of cost_volume_analysis.py.

The bound on mean_rest (cv_probe_ref.rounding_bound): the fp32 sum of D values is off by at most one rounding per addition, each
at most 2^-24 of a partial sum that sum |v| bounds; two subtractions the same; the division by D - 2 scales that and adds one
rounding of the quotient: (D + 2) * 2^-24 * sum |v| / (D - 2) + 2^-24 * |mean_rest|.  The reference's own fp32 mean of D - 2 values
obeys the same bound, so the two fp32 values are within twice it of each other.
"""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cv_probe_ref as R
import ood_ref
from adaptive_stereo import _native as nat
from conftest import GOLDEN_DIR, REPO, parity_note


@pytest.fixture(scope="module")
def fixture():
  return np.load(os.path.join(GOLDEN_DIR, "cv_probe.npz"), allow_pickle=False)


@pytest.mark.parametrize("name", R.STORED_NAMES)
def test_restatement_against_the_reference(fixture, name):
  vol, gt, forced = R.make_case(name)
  B, D, H, W = vol.shape
  assert np.array_equal(ood_ref.checksum(vol), fixture["check__" + name])
  got = R.probe(vol, gt)
  picks = fixture["pick__" + name]
  assert np.array_equal(got["p"], picks), "picks differ from torch.argmax / argmin of the reference's map"
  assert np.array_equal(got["pix"][..., 0], picks // W) and np.array_equal(got["pix"][..., 1], picks % W)
  for (b, which), p in forced.items():
    assert got["p"][b, which] == p, "the planted pick"
  flat = vol.reshape(B, D, H * W)
  worst = 0.0
  for b in range(B):
    for which in range(2):
      p = int(picks[b, which])
      column = flat[b, :, p]
      assert np.array_equal(R.bits(got["slices"][b, which]), R.bits(column)), "the slice is not the pixel's logits bit for bit"
      f, m1, m2, mean_rest, g = got["vals"][b, which]
      assert R.bits(g) == R.bits(gt.reshape(B, -1)[b, p])
      if np.isnan(column).any():
        assert np.isnan(vol[b]).any() and got["pix"][b, which, 2] == -1
        assert all(R.bits(x) == 0x7FC00000 for x in (f, m1, m2, mean_rest))
        continue
      assert R.bits(m1) == R.bits(fixture["max__" + name][b, which]), "m1 is not sorted[0]"
      assert column[got["pix"][b, which, 2]] == m1 and not (column[:got["pix"][b, which, 2]] == m1).any(), "d_max"
      assert m2 == np.sort(column)[-2]
      bound, exact = R.rounding_bound(column)
      assert abs(float(mean_rest) - exact) <= bound
      assert abs(float(mean_rest) - float(fixture["mean__" + name][b, which])) <= 2 * bound
      worst = max(worst, abs(float(mean_rest) - exact) / bound)
      assert R.bits(f) == R.bits(np.float32(m1 - mean_rest)), "f != m1 - mean_rest bit for bit"
  parity_note("cv_probe_ref_mean_rest_" + name, worst_share_of_bound=worst)


@pytest.mark.parametrize("name", [n for n in R.CASE_NAMES if n not in R.STORED_NAMES] + ["b2_d12_h5_w67_g1", "b1_d64_h2_w70_g50"])
def test_profile_is_the_exact_rank_mean_and_small_d_rules(name):
  """The profile against an independent computation: Python's sorted() per pixel and math.fsum per rank, rounded once.  The
  D <= 2 cases (not in the fixture: the reference's map is NaN there): the map is 0, both picks are pixel 0, mean_rest is NaN."""
  vol, gt, _ = R.make_case(name)
  B, D, H, W = vol.shape
  got = R.probe(vol, gt)
  for b in range(B):
    cols = vol[b].reshape(D, -1).T.tolist()
    if np.isnan(vol[b]).any():
      assert np.isnan(got["profile"][b]).all()
      continue
    ranked = [sorted(c, reverse=True) for c in cols]
    want = np.array([math.fsum(r[j] for r in ranked) / len(cols) for j in range(D)]).astype(np.float32)
    assert np.array_equal(got["profile"][b], want)
    if D <= 2:
      assert got["p"][b].tolist() == [0, 0] and not got["vals"][b, :, 0].any()
      assert (R.bits(got["vals"][b, :, 3]) == 0x7FC00000).all()
      assert np.array_equal(got["vals"][b, :, 1], [vol[b, :, 0, 0].max()] * 2)
      assert np.array_equal(got["vals"][b, :, 2], [vol[b, :, 0, 0].min() if D == 2 else -np.inf] * 2)


def test_pixel_worked_by_hand():
  """values 1, 7, 3, 7, -2: m1 = m2 = 7 (the first 7, d = 1), sum 16, mean_rest (16 - 7 - 7) / 3 = 2/3, f = 7 - 2/3."""
  f, m1, m2, mean_rest, d_max = R.pixel_values(np.array([1, 7, 3, 7, -2], np.float32))
  assert (m1, m2, d_max) == (7.0, 7.0, 1)
  assert mean_rest == np.float32(2) / np.float32(3) and f == np.float32(7) - np.float32(2) / np.float32(3)
  assert R.select(np.array([[0.0, 3.0], [3.0, -0.0]], np.float32)) == (1, 0)           # first of the ties; -0 equals +0
  assert R.select(np.array([[5.0, np.nan], [np.nan, -1.0]], np.float32)) == (1, 1)     # the first NaN, both times
  without_gt = R.probe(np.zeros((1, 3, 1, 2), np.float32))
  assert (R.bits(without_gt["vals"][..., 4]) == 0x7FC00000).all()


def test_bad_arguments_are_refused_before_any_launch():
  """No GPU needed: every one of these returns before the first launch, with a message that names the argument."""
  lib = nat.load()
  fake = ctypes.c_void_p(4096)              # never dereferenced
  def call(logits=fake, gt=None, B=1, D=12, H=2, W=3, pix=fake, vals=fake, slices=fake, profile=fake, capacity=4, cursor=None,
           dropped=None):
    return lib.as_cost_volume_probe(logits, gt, B, D, H, W, pix, vals, slices, profile, capacity, cursor, dropped, None)
  assert call(D=65) != 0 and b"D 65" in lib.as_last_error()
  assert call(D=0) != 0 and b"D 0" in lib.as_last_error()
  assert call(B=0) != 0 and b"B 0" in lib.as_last_error()
  assert call(B=65536) != 0 and b"B 65536" in lib.as_last_error()
  assert call(H=1 << 15, W=(1 << 15) + 1) != 0 and b"H 32768" in lib.as_last_error()
  assert call(capacity=0) != 0 and b"capacity 0" in lib.as_last_error()
  assert call(pix=None, vals=None, slices=None, profile=None) != 0 and b"no output" in lib.as_last_error()
  assert call(pix=None, vals=None, slices=None, profile=None, cursor=fake) != 0 and b"cursor" in lib.as_last_error()
  assert call(logits=None) != 0 and b"as_cost_volume_probe" in lib.as_last_error()


def test_python_layer_refuses_what_cannot_run():
  from adaptive_stereo import cv_probe
  with pytest.raises(ValueError, match="capacity"):
    cv_probe.CostVolumeProbe(0, 12)
  with pytest.raises(ValueError, match="D 65"):
    cv_probe.CostVolumeProbe(4, 65)
  with pytest.raises(RuntimeError, match="no CPU path"):
    cv_probe.CostVolumeProbe(4, 12, device="cpu")
  with pytest.raises(RuntimeError, match="no CPU path"):
    cv_probe.probe_cost_volume(torch.zeros(1, 12, 2, 3))


def test_sorting_network_sorts_on_the_host(tmp_path):
  """csrc/sort_net.h by the 0-1 principle (tests/tools/sort_net_check.cpp): exhaustive up to N = 16, sampled beyond."""
  if shutil.which("g++") is None:
    pytest.skip("no g++")
  exe = str(tmp_path / "sort_net_check")
  subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(REPO, "tests", "tools", "sort_net_check.cpp"), "-o", exe], check=True)
  out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
  assert out.returncode == 0, out.stdout + out.stderr
  assert "N 64: 543 comparators" in out.stdout


def test_curve_data_is_what_the_figure_shows():
  """cost_volume_analysis.curve_data on a hand-made probes dict: train reads the "hi" pick, novel the "lo" pick."""
  import cost_volume_analysis as cva
  vals = torch.tensor([[[5.0, 9.0, 8.0, 4.0, 2.5], [0.5, 3.0, 2.0, 2.5, 1.0]]])
  probes = dict(pix=torch.tensor([[[1, 2, 3], [4, 5, 0]]], dtype=torch.int32), vals=vals,
                slices=torch.arange(8.0).reshape(1, 2, 4), profile=torch.zeros(1, 4))
  hi = cva.curve_data(probes, 0, "hi")
  assert hi["curve"].tolist() == [0.0, 1.0, 2.0, 3.0] and hi["disparity"] == [0, 1, 2, 3]
  assert (hi["max"], hi["mean_rest"], hi["gt"], hi["fcs"]) == (9.0, 4.0, 2.5, 5.0) and (hi["row"], hi["col"], hi["d_max"]) == (1, 2, 3)
  lo = cva.curve_data(probes, 0, "lo")
  assert lo["curve"].tolist() == [4.0, 5.0, 6.0, 7.0] and (lo["max"], lo["mean_rest"], lo["gt"]) == (3.0, 2.5, 1.0)
  assert cva.DOMAIN_PICK == {"train": "hi", "novel": "lo"}
  with pytest.raises(ValueError):
    cva.curve_data(probes, 0, "middle")
  with pytest.raises(IndexError):
    cva.curve_data(probes, 1, "hi")
  with pytest.raises(NotImplementedError):
    cva.main(["--debug"])
  with pytest.raises(NotImplementedError):
    cva.main([])
  with pytest.raises(SystemExit):
    cva.main(["--save"])                                   # --save without the dataset flags and the weights

