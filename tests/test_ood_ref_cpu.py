"""tests/ood_ref.py — the host restatement that tests/test_gpu_ood.py compares csrc/ood.hip against — and the host half of
adaptive_stereo/ood.py (threshold, precision/recall sweep, monotone post-process, histogram), held to things that do not depend
on them: the reference's own maps (tests/golden/ood_fcs.npz), scipy's inverse normal cdf, a plain double loop, and small cases
worked by hand."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ood_ref as R
from adaptive_stereo import ood
from conftest import GOLDEN_DIR, parity_note

CASES = [(shape, gain) for shape in R.SHAPES for gain in R.GAINS]
IDS = [R.case_name(s, g) for s, g in CASES]


@pytest.fixture(scope="module")
def fixture():
  return np.load(os.path.join(GOLDEN_DIR, "ood_fcs.npz"), allow_pickle=False)


@pytest.mark.parametrize("shape,gain", CASES, ids=IDS)
def test_volume_regenerates_and_median_by_rank_equals_the_reference(fixture, shape, gain):
  """The regenerated volume has the stored fingerprint; the rank-selected median map equals the reference's
  max - torch.median exactly (==, NaN by position), planted pixels included."""
  vol = R.make_volume(shape, gain)
  name = R.case_name(shape, gain)
  assert np.array_equal(R.checksum(vol), fixture["check__" + name])
  want = fixture["median__" + name]
  got = R.fcs_median(vol)
  assert got.dtype == np.float32 and R.same_values(got, want)
  for kind, (b, p) in R.planted(shape).items():
    g, w = got.reshape(shape[0], -1)[b, p], want.reshape(shape[0], -1)[b, p]
    assert (np.isnan(g) and np.isnan(w)) if kind == "nan" else g == w, kind
  if "all_equal" in R.planted(shape):
    assert got.reshape(shape[0], -1)[0, 0] == 0.0 and got.reshape(shape[0], -1)[0, 3] == 0.0      # all equal; all zeros


@pytest.mark.parametrize("shape,gain", [c for c in CASES if c[0][1] > 2], ids=[i for c, i in zip(CASES, IDS) if c[0][1] > 2])
def test_mean_formula_is_the_reference_sorted_mean_within_the_existing_bar(fixture, shape, gain):
  """m1 - (sum - m1 - m2)/(D-2) with its in-order fp32 sum against the reference's max - mean(sorted[2:]): the bar of
  test_out_conv_softargmax_fcs for the same comparison, 1e-5 * max(1, gain) absolute + 1e-5 relative; NaN by position."""
  vol = R.make_volume(shape, gain)
  want = fixture["mean__" + R.case_name(shape, gain)].astype(np.float64)
  got = R.fcs_mean(vol).astype(np.float64)
  assert np.array_equal(np.isnan(got), np.isnan(want))
  ok = ~np.isnan(want)
  err = np.abs(got[ok] - want[ok])
  parity_note("ood_ref_mean_vs_reference_" + R.case_name(shape, gain), worst_abs=float(err.max()))
  assert bool((err <= 1e-5 * max(1.0, gain) + 1e-5 * np.abs(want[ok])).all())


def test_mean_formula_small_d_and_worked_pixel():
  """D <= 2 gives 0 (the reference: NaN, the mean of an empty slice); one pixel worked by hand: values 1, 7, 3, 7, -2 ->
  m1 = m2 = 7, sum 16, 7 - (16 - 7 - 7)/3 = 7 - 2/3; median: rank 2 of (-2, 1, 3, 7, 7) is 3 -> 4."""
  for D in (1, 2):
    vol = np.arange(D * 4, dtype=np.float32).reshape(1, D, 2, 2)
    assert not R.fcs_mean(vol).any()
    assert R.same_values(R.fcs_median(vol), (vol.max(axis=1) - vol.min(axis=1)))     # D = 2: lower median = min; D = 1: 0
  vol = np.array([1, 7, 3, 7, -2], np.float32).reshape(1, 5, 1, 1)
  assert R.fcs_mean(vol)[0, 0, 0] == np.float32(7) - np.float32(2) / np.float32(3)
  assert R.fcs_median(vol)[0, 0, 0] == 4.0


def test_image_scores_are_the_fp64_mean_rounded_once():
  a = np.array([[[0.1, 0.2], [0.3, 16777216.0]], [[1.0, 2.0], [3.0, np.nan]]], np.float32)
  got = R.image_scores(a, a * np.float32(2))
  want0 = np.float32(math.fsum(float(v) for v in a[0].ravel()) / 4.0)
  assert got.shape == (2, 2) and got.dtype == np.float32
  assert got[0, 0] == want0 and got[0, 1] == np.float32(2) * want0
  assert np.isnan(got[1]).all()
  assert R.ulp_gap(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1.0


# ---- csrc/column_stats.h on the host ------------------------------------------------------------------------------------
COLUMN_DS = (1, 2, 3, 4, 5, 12, 13, 24, 25, 64)


def designed_columns(D):
  """[n, D] fp32, one pattern per row: the maximum twice, all equal, ascending, descending, zeros of both signs (starting with
  either), one -inf, values at gain 20 (the order of the fp32 sum shows), a NaN first, a NaN last."""
  rs = np.random.RandomState(4242 + D)
  f = np.float32
  ramp = (np.arange(D, dtype=np.float32) - f(D // 2)) * f(0.7)
  twice = rs.standard_normal(D).astype(np.float32)
  twice[0] = twice[D - 1] = np.abs(twice).max() + f(1)
  zeros = np.where(np.arange(D) % 2 == 0, f(0.0), f(-0.0)).astype(np.float32)
  minf = rs.standard_normal(D).astype(np.float32)
  minf[D // 2] = -np.inf
  rows = [twice, np.full(D, 1.5, np.float32), ramp, ramp[::-1], zeros, -zeros, minf]
  rows += [(rs.standard_normal(D) * 20.0).astype(np.float32) for _ in range(4)]
  for at in (0, D - 1):
    v = (rs.standard_normal(D) * 20.0).astype(np.float32)
    v[at] = np.nan
    rows.append(v)
  return np.stack(rows)


@pytest.fixture(scope="module")
def column_stats_exe(tmp_path_factory):
  if shutil.which("g++") is None:
    pytest.skip("no g++")
  exe = str(tmp_path_factory.mktemp("column_stats") / "column_stats_check")
  src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "column_stats_check.cpp")
  subprocess.run(["g++", "-O2", "-std=c++17", src, "-o", exe], check=True)
  return exe


@pytest.mark.parametrize("D", COLUMN_DS)
def test_column_stats_header_is_the_restatement(column_stats_exe, tmp_path, D):
  """col_top2_step and col_fcs of csrc/column_stats.h, compiled for the host, over designed columns: the fcs bits are
  ood_ref.fcs_mean's (which is held to the reference's fixture above), am is numpy's first arg-max, m1 and m2 the two largest
  values; a column with a NaN sets has_nan, for which ood_ref's rule (the map is NaN) is the callers' to apply."""
  cols = designed_columns(D)
  n = cols.shape[0]
  path = str(tmp_path / "columns.txt")
  with open(path, "w") as f:
    f.write("%d %d\n" % (n, D))
    for row in cols.view(np.uint32):
      f.write(" ".join("%08x" % u for u in row) + "\n")
  out = subprocess.run([column_stats_exe, path], capture_output=True, text=True, timeout=60)
  assert out.returncode == 0, out.stdout + out.stderr
  lines = out.stdout.split("\n")[:-1]
  assert len(lines) == n
  want = R.fcs_mean(np.ascontiguousarray(cols.T).reshape(1, D, 1, n))[0, 0]
  for i, line in enumerate(lines):
    fcs, m1, m2, am, has_nan = line.split()
    col = cols[i]
    assert int(has_nan) == int(np.isnan(col).any()), i
    if int(has_nan):
      assert np.isnan(want[i])
      col = np.where(np.isnan(col), np.float32(-np.inf), col)        # a NaN compares false: it never becomes the maximum
    else:
      assert int(fcs, 16) == int(want[i:i + 1].view(np.uint32)[0]), (i, fcs, want[i])
    top = np.sort(np.concatenate([col, np.full(1, -np.inf, np.float32)]))[::-1]
    assert int(am) == int(np.argmax(col)), i
    got = np.array([int(m1, 16), int(m2, 16)], np.uint32).view(np.float32)
    assert got[0] == top[0] and got[1] == top[1], (i, got, top[:2])
  if D >= 2:
    assert lines[0].split()[1] == lines[0].split()[2] and lines[0].split()[3] == "0"      # the maximum twice: m2 == m1, first index


def test_row_cursor_refuses_before_any_device_call():
  from adaptive_stereo import collect
  with pytest.raises(ValueError, match="capacity 0 must be at least 1"):
    collect.RowCursor("X", 0, "cuda")
  with pytest.raises(RuntimeError, match="no CPU path"):
    collect.RowCursor("X", 1, "cpu")


# ---- threshold ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("percentile", [0.01, 0.05, 0.3, 0.5, 0.95, 0.99])
def test_threshold_is_scipy_norm_ppf(percentile):
  stats = pytest.importorskip("scipy.stats")
  x = (12.0 + 1.5 * np.random.RandomState(7).standard_normal(200)).astype(np.float32)
  thr, mu, sigma = ood.ood_threshold(torch.from_numpy(x), percentile)
  x64 = x.astype(np.float64)
  assert mu == x64.mean() and sigma == math.sqrt(x64.var(ddof=1))
  want = float(stats.norm.ppf(percentile, loc=mu, scale=sigma))
  assert abs(thr - want) <= 1e-12 * abs(want)
  assert ood.ood_threshold(x, percentile) == (thr, mu, sigma)            # numpy and lists are taken as well


def test_threshold_at_the_fixture_scores_is_the_reference_formula(fixture):
  """The reference takes mu and var from torch in fp32; ours are fp64.  An fp32 mean or unbiased variance of n = 64 values is
  off by at most n * 2^-24 relative (pairwise or not), so the thresholds differ by at most 64 * 2^-24 * (|mu| + |z| * sigma)."""
  scores = torch.from_numpy(fixture["scores"])
  for p, want in zip(fixture["percentiles"], fixture["thresholds"]):
    thr, mu, sigma = ood.ood_threshold(scores, float(p))
    z = (thr - mu) / sigma
    bound = 64 * 2.0 ** -24 * (abs(mu) + abs(z) * sigma)
    parity_note("ood_threshold_vs_reference_p%g" % p, got=thr, want=float(want), bound=bound)
    assert abs(thr - float(want)) <= bound
  assert abs(ood.ood_threshold(scores, 0.5)[0] - ood.ood_threshold(scores, 0.5)[1]) == 0.0      # the median of a normal: mu


def test_argument_errors():
  x = torch.rand(8)
  for p in (0.0, 0.009, 0.991, 1.0, float("nan")):
    with pytest.raises(ValueError, match="percentile"):
      ood.ood_threshold(x, p)
  with pytest.raises(ValueError, match="non-empty"):
    ood.ood_threshold(torch.zeros(0), 0.05)
  with pytest.raises(ValueError, match="non-empty"):
    ood.precision_recall(x, torch.zeros(0))
  with pytest.raises(ValueError, match="non-empty"):
    ood.precision_recall(torch.zeros(0), x)
  with pytest.raises(ValueError, match="non-empty"):
    ood.fcs_histogram(torch.zeros(0), x)
  with pytest.raises(ValueError, match="1-D"):
    ood.precision_recall(torch.rand(2, 2), x)
  assert math.isnan(ood.ood_threshold(torch.ones(1), 0.05)[2])          # one score: no variance


# ---- the sweep ----------------------------------------------------------------------------------------------------------
def check_sweep(train, novel, num):
  got = ood.precision_recall(torch.as_tensor(train), torch.as_tensor(novel), num)
  want = R.precision_recall_loop(train, novel, num)
  assert got["cutoffs"].dtype == np.float32 and np.array_equal(got["cutoffs"], np.array(want["cutoffs"], np.float32))
  for k in ("tp", "fn", "tn", "fp"):
    assert got[k].dtype == np.int64 and got[k].tolist() == want[k], k
  assert got["precision"].dtype == got["recall"].dtype == np.float64
  assert got["precision"].tolist() == want["precision"] and got["recall"].tolist() == want["recall"]
  return got


@pytest.mark.parametrize("n", [1, 7, 1000])
def test_precision_recall_is_the_double_loop(n):
  rs = np.random.RandomState(n)
  novel = (10.0 + 2.0 * rs.standard_normal(n)).astype(np.float32)
  train = (13.0 + 1.5 * rs.standard_normal(max(n, 3))).astype(np.float32)
  got = check_sweep(train, novel, 100)
  assert got["tp"][-1] == n and got["fn"][-1] == 0 and got["tp"][0] >= 1          # the ends are the novel set's min and max


def test_cutoff_that_rounds_up_onto_a_score_counts_it():
  """novel = {0, v}, four cutoffs 0, v/3, 2v/3, v: v/3 is no fp32 number, and v is the first fp32 value from 0.3 upward whose
  fp64 third rounds UP to fp32.  A training score equal to that fp32 value lies above the fp64 cutoff and on the fp32 one."""
  v = np.float32(0.3)
  while not float(np.float32(np.linspace(0.0, float(v), 4)[1])) > np.linspace(0.0, float(v), 4)[1]:
    v = np.nextafter(v, np.float32(1))
  cut64 = np.linspace(0.0, float(v), 4)[1]
  score = np.float32(cut64)
  assert float(score) > cut64
  novel = np.array([0.0, v], np.float32)
  train = np.array([score, 1.0], np.float32)
  got = check_sweep(train, novel, 4)
  assert got["fp"].tolist() == [0, 1, 1, 1]                    # the fp32 compare counts it from the second cutoff on
  assert int((train.astype(np.float64) <= cut64).sum()) == 0   # an fp64 compare would not have


def test_precision_is_one_where_nothing_is_called_novel():
  """tp + fp == 0: every cutoff is at least the novel set's minimum, which is then called novel, so with finite scores the
  case cannot arise; a novel set whose only score is NaN compares false everywhere and reaches it."""
  got = ood.precision_recall(torch.tensor([1.0, 2.0]), torch.tensor([float("nan")]), 4)
  assert got["tp"].tolist() == [0] * 4 and got["fp"].tolist() == [0] * 4
  assert got["precision"].tolist() == [1.0] * 4 and got["recall"].tolist() == [0.0] * 4
  assert got["fn"].tolist() == [1] * 4 and got["tn"].tolist() == [2] * 4


# ---- post-process and histogram -------------------------------------------------------------------------------------------
def test_strictly_decreasing_precision_by_hand():
  """recall 0.2, 0.4, 0.6, 0.8, 1.0 with precision 0.9, 0.5, 0.7, 0.3, 0.4: from the right the running maximum is
  0.4, 0.4, 0.7, 0.7, 0.9 -> read left to right 0.9, 0.7, 0.7, 0.4, 0.4.  Given out of order to show the sort."""
  re = np.array([0.6, 0.2, 1.0, 0.4, 0.8])
  pr = np.array([0.7, 0.9, 0.4, 0.5, 0.3])
  r, p = ood.strictly_decreasing_precision(pr, re)
  assert r.tolist() == [0.2, 0.4, 0.6, 0.8, 1.0]
  assert p.tolist() == [0.9, 0.7, 0.7, 0.4, 0.4]
  assert bool((np.diff(p) <= 0).all())
  with pytest.raises(ValueError):
    ood.strictly_decreasing_precision(pr, re[:3])


def test_histogram_by_hand():
  """train {0, 1, 1, 4}, novel {2, 8}, 4 bins: edges 0, 2, 4, 6, 8 over both sets; train counts 3, 0, 1, 0 -> densities
  3/8, 0, 1/8, 0 (count / (n * width)); novel counts 0, 1, 0, 1 (2 opens the second bin, 8 closes the last) -> 0, 1/4, 0, 1/4."""
  edges, dt, dn = ood.fcs_histogram(torch.tensor([0.0, 1.0, 1.0, 4.0]), torch.tensor([2.0, 8.0]), bins=4)
  assert edges.tolist() == [0.0, 2.0, 4.0, 6.0, 8.0]
  assert dt.tolist() == [0.375, 0.0, 0.125, 0.0]
  assert dn.tolist() == [0.0, 0.25, 0.0, 0.25]
  edges, dt, dn = ood.fcs_histogram(np.arange(50, dtype=np.float32), np.arange(30, 90, dtype=np.float32))
  assert len(edges) == 41 and edges[0] == 0.0 and edges[-1] == 89.0
  assert abs((dt * np.diff(edges)).sum() - 1.0) < 1e-12 and abs((dn * np.diff(edges)).sum() - 1.0) < 1e-12
