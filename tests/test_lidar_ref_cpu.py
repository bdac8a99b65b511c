"""tests/lidar_ref.py (the numpy restatement that the GPU tests compare csrc/lidar.hip with) against the REFERENCE's own outputs,
tests/golden/lidar_gt.npz, which tests/golden/make_golden_lidar.py produced by running scripts/export_gt_disp.py itself.

Bit for bit on columns 1..W-2.  Columns 0 and W-1 are left out, and only they: the reference's duplicate search merges pixel
(r, W-1) with pixel (r+1, 0) (lidar_ref's docstring); how many of their pixels differ is reported, not asserted.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, parity_note
import lidar_ref as R

F = np.float32
CASES = [(name, cam, vd) for name in sorted(R.SCANS) for cam in (2, 3) for vd in (0, 1)]


@pytest.fixture(scope="module")
def fixture():
  return np.load(os.path.join(GOLDEN_DIR, "lidar_gt.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def scans():
  return {name: R.make_scan(name) for name in R.SCANS}


def _bits(a):
  return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def test_inputs_regenerate(fixture, scans):
  assert "numpy" in str(fixture["meta"])
  for name, scan in scans.items():
    H, W, N, _ = R.SCANS[name]
    assert scan.shape == (N, 4) and scan.dtype == F
    assert tuple(fixture["shape__" + name]) == (H, W)
    assert np.array_equal(R.checksum(scan), fixture["check__scan__" + name]), name
  g = scans["general"]
  assert np.isnan(g[:, 0]).any() and np.isposinf(g[:, 0]).any() and (g[:, 0] < 0).any()
  assert np.signbit(g[g[:, 0] == 0, 0]).any()                                  # the -0.0
  assert int(fixture["behind__general"]) >= 4                                  # in-bounds points with q2 < 0, over both cameras


def test_projection_matrices_match_the_reference(fixture):
  for name in R.SCANS:
    P = R.projections(name)
    for cam in (2, 3):
      assert np.array_equal(P[cam], fixture["P%d__%s" % (cam, name)]), (name, cam)
    assert R.file_calibration(name)["P_rect_02"][0, 0] == float(fixture["fx__" + name])
    assert not np.array_equal(P[2][:, 3], P[3][:, 3])


def test_calibration_parser_matches_the_reference(fixture, tmp_path):
  from adaptive_stereo.lidar import KittiCalibration, read_calib_file
  for name in R.SCANS:
    d = str(tmp_path / name)
    R.write_calibration(d, name)
    raw = read_calib_file(os.path.join(d, "calib_cam_to_cam.txt"))
    assert raw["calib_time"] == "09-Jan-2012 13:57:47" and raw["rig"] == "synthetic " + name      # first colon only; text stays text
    assert raw["corner_dist"].shape == (1,) and raw["P_rect_03"].shape == (12,)
    calib = KittiCalibration.from_files(d)
    for cam in (2, 3):
      assert calib.velo_to_image(cam).dtype == np.float64
      assert np.array_equal(calib.velo_to_image(cam), fixture["P%d__%s" % (cam, name)]), (name, cam)
    assert calib.image_shape == tuple(fixture["shape__" + name])
    assert calib.fx == float(fixture["fx__" + name]) and calib.baseline == 0.54
    assert calib.bf == R.bf(name)
  direct = KittiCalibration(fixture["P2__general"], fixture["P3__general"], (75, 131), 98.7)
  assert np.array_equal(direct.velo_to_image(3), fixture["P3__general"])
  with pytest.raises(ValueError):
    KittiCalibration(np.zeros((3, 3)), np.zeros((3, 4)), (75, 131), 98.7)


@pytest.mark.parametrize("name,cam,vd", CASES)
def test_depth_map_equals_the_reference_off_the_edge_columns(fixture, scans, name, cam, vd):
  H, W = R.SCANS[name][:2]
  want = fixture["depth__%s__cam%d__vd%d" % (name, cam, vd)]
  assert want.dtype == np.float64
  got = R.depth_map(R.projections(name)[cam], scans[name], (H, W), bool(vd))
  with np.errstate(over="ignore"):
    want32 = want.astype(F)
  assert (got > 0).sum() > H * W // 20                                           # the scan really covers the image
  diff = _bits(got) != _bits(want32)
  assert not diff[:, 1:W - 1].any(), "%d interior pixels differ, first %r" % (
      int(diff[:, 1:W - 1].sum()), (np.argwhere(diff[:, 1:W - 1])[0] + [0, 1]).tolist())
  parity_note("lidar_ref_depth_vs_reference_%s_cam%d_vd%d" % (name, cam, vd), edge_column_pixels_differing=int(diff.sum()),
              of=2 * H, valid=int((got > 0).sum()))


@pytest.mark.parametrize("name,cam", [(n, c) for n in sorted(R.SCANS) for c in (2, 3)])
def test_export_equals_the_reference_off_the_edge_columns(fixture, scans, name, cam):
  H, W = R.SCANS[name][:2]
  want = fixture["export__%s__cam%d" % (name, cam)]
  assert want.dtype == np.uint16 and want.shape == (H, W)
  depth = R.depth_map(R.projections(name)[cam], scans[name], (H, W), True)
  _, disp, q, over = R.disparity(depth, R.bf(name), quantize=True)
  assert over == 0
  diff = q != want
  assert not diff[:, 1:W - 1].any(), "%d interior pixels differ" % int(diff[:, 1:W - 1].sum())
  assert np.array_equal(_bits(disp), _bits(q.astype(F) * F(1.0 / 128)))          # what the dataset layer decodes from the file
  assert (q[depth > F(80)] == 0).all() and (q > 0).sum() > H * W // 20
  parity_note("lidar_ref_export_vs_reference_%s_cam%d" % (name, cam), edge_column_pixels_differing=int(diff.sum()), of=2 * H)


def test_dyadic_scan_sits_on_the_rounding_edge(fixture, scans):
  """Most of its q0/q2 are exactly k + 0.5, for even and odd k: rounding half away from zero puts them elsewhere."""
  H, W = R.SCANS["dyadic"][:2]
  rows, cols, q2, x, a, b = R.project(R.projections("dyadic")[2], scans["dyadic"], (H, W))
  half = (a - np.floor(a)) == 0.5
  assert half.sum() > 500 and (np.floor(a[half]) % 2 == 0).any() and (np.floor(a[half]) % 2 == 1).any()
  away = np.floor(a + 0.5) - 1.0
  assert (away != cols).sum() > 100                                              # round() instead of rint would move these points


def test_metrics_restatement_counts():
  gt = np.array([0, 1, 2, 3, 4, 5, 6], dtype=F)
  pred = gt + np.array([9, 2, 2.5, 3, -4.5, 5, -6], dtype=F)                     # strict >: 2, 3 and 5 exactly do not count
  s, counts = R.metrics(pred, gt)
  assert counts == [6, 5, 3, 3, 1] and s == 23.0
