"""tests/rectify_ref.py and the host side of adaptive_stereo.rectify, without a GPU.

The fp32 restatement (what the kernels are held to bit for bit) is pinned against the fp64 one: on the maps by a bound measured
here from the two references and given x4 (rectify_ref.MAP_BOUND), on the images by a derived one: a bilinear sample is Lipschitz
in its coordinates, the slopes being at most the largest differences Lx, Ly of horizontally and vertically adjacent taps, so
|out32 - out64| <= (|d us| * Lx + |d vs| * Ly) / 255 + 4 ulp.  The geometry is pinned through the fp64 map against the forward
camera model: no iteration anywhere, so 1e-8 px is fp64 rounding."""
import os
import re

import numpy as np
import pytest

import rectify_ref as rr
from conftest import PKG
from adaptive_stereo import rectify as rx

F = np.float32


def view_calib(view, raw=None, window=None):
  """a rectify_ref.Calib of an adaptive_stereo.rectify.RectifiedView"""
  K, P = view.raw.K, view.P
  assert P[0, 0] == P[1, 1]
  return rr.Calib((K[0, 0], K[1, 1], K[0, 2], K[1, 2]), view.raw.D, view.R, (P[0, 0], P[0, 2], P[1, 2]), P[0, 3],
                  view.raw.size if raw is None else raw, (0, 0) + tuple(view.size) if window is None else window)


def calib_view(cal):
  raw = rx.RawCamera(cal.K_matrix(), cal.D, cal.raw)
  return rx.RectifiedView(raw, cal.R, cal.P_matrix(), cal.window[2:])


def test_the_references_tile_constants_are_the_kernels():
  text = open(os.path.join(PKG, "csrc", "rectify.hip")).read()
  define = lambda name: re.search(r"#define %s\s+(\S+)" % name, text).group(1)
  assert int(define("RC_PX")) == rr.RC_PX and int(define("RC_ROWS")) == rr.RC_ROWS and int(define("RC_LANES")) * rr.RC_PX == rr.RC_SPAN


@pytest.mark.parametrize("name", ["KITTI_LIKE", "KITTI_LIKE_R", "RATIONAL"])
def test_fp32_maps_against_fp64(name):
  cal = rr.CALIBS[name]
  a = rr.rectify_map(cal, cal.raw, cal.window, F)
  b = rr.rectify_map(cal, cal.raw, cal.window, np.float64)
  both = a[2] & b[2]
  worst = max(float(np.abs(a[0].astype(np.float64) - b[0])[both].max()), float(np.abs(a[1].astype(np.float64) - b[1])[both].max()))
  print("%s: max |map32 - map64| = %.3e px over %d pixels valid in both (bound %.3e)" % (name, worst, int(both.sum()), rr.MAP_BOUND))
  assert both.mean() > 0.7
  assert worst <= rr.MAP_BOUND
  if name.startswith("KITTI"):
    assert a[2].all() and b[2].all()           # the contract alone keeps the whole 375 x 1242 window valid
  # where the two disagree on validity the fp64 coordinate is within the bound of the raw border
  H0, W0 = cal.raw
  near = (np.abs(b[0]) <= rr.MAP_BOUND) | (np.abs(b[0] - (W0 - 1)) <= rr.MAP_BOUND) | (np.abs(b[1]) <= rr.MAP_BOUND) | \
         (np.abs(b[1] - (H0 - 1)) <= rr.MAP_BOUND)
  assert not ((a[2] != b[2]) & ~near).any()
  assert near.mean() <= 1e-3


@pytest.mark.parametrize("name,C", [("KITTI_LIKE", 3), ("RATIONAL", 3), ("QUARTER", 1)])
def test_fp32_images_against_fp64_within_the_lipschitz_bound(name, C):
  cal = rr.CALIBS[name]
  H0, W0 = cal.raw
  src = rr.random_raw(1, cal.raw, C, 5)
  a = rr.rectify_map(cal, cal.raw, cal.window, F)
  b = rr.rectify_map(cal, cal.raw, cal.window, np.float64)
  out32 = rr.sample(src, *a, fill=0.25, dtype=F)
  out64 = rr.sample(src, *b, fill=0.25, dtype=np.float64)
  assert out32.dtype == F and out32.shape == (1, 3) + tuple(cal.window[2:])
  s = src.astype(np.float64)
  Lx, Ly = np.abs(np.diff(s, axis=2)).max(), np.abs(np.diff(s, axis=1)).max()
  near = (np.abs(b[0]) <= rr.MAP_BOUND) | (np.abs(b[0] - (W0 - 1)) <= rr.MAP_BOUND) | (np.abs(b[1]) <= rr.MAP_BOUND) | \
         (np.abs(b[1] - (H0 - 1)) <= rr.MAP_BOUND)
  assert near.mean() <= 1e-3                   # at most 0.1 % of the pixels are left out
  keep = ~near
  assert np.array_equal(a[2][keep], b[2][keep])
  with np.errstate(invalid="ignore"):
    dus = np.where(b[2], np.abs(a[0].astype(np.float64) - b[0]), 0.0)
    dvs = np.where(b[2], np.abs(a[1].astype(np.float64) - b[1]), 0.0)
  bound = (dus * Lx + dvs * Ly) / 255.0 + 4 * rr.ULP1
  err = np.abs(out32.astype(np.float64) - out64)
  worst = float((err / bound[None, None])[:, :, keep].max())
  print("%s: max |out32 - out64| = %.3e, at most %.3f of the derived bound; %d of %d pixels left out"
        % (name, float(err[:, :, keep].max()), worst, int(near.sum()), near.size))
  assert worst <= 1.0
  assert np.array_equal(out32[:, :, ~a[2]], np.full_like(out32[:, :, ~a[2]], 0.25))       # fill, in every plane
  if C == 1:
    assert np.array_equal(out32[:, 0], out32[:, 1]) and np.array_equal(out32[:, 0], out32[:, 2])


def test_the_horizon_calibrations_give_nan_infinite_and_huge_coordinates():
  cal = rr.HORIZON
  us, vs, valid = rr.rectify_map(cal, cal.raw, cal.window)
  m = cal.inverse()
  u, v = rr.grid(cal.window, np.float64)
  Z = m[2, 0] * u + m[2, 1] * v + m[2, 2]
  assert (Z > 0.01).any() and (Z < -0.01).any()               # Z changes sign inside the window
  assert np.isnan(us).any() and not valid[np.isnan(us)].any()
  us_b, vs_b, valid_b = rr.rectify_map(rr.HORIZON_B, cal.raw, cal.window)
  assert np.isinf(us_b).any() and (np.abs(us_b[np.isfinite(us_b)]) > 2.0 ** 31).any()
  assert not valid_b[~np.isfinite(us_b)].any()
  assert 0.1 < valid.mean() < 0.9 and 0.1 < valid_b.mean() < 0.9
  # and the sampler never converts such a coordinate
  out = rr.sample(rr.random_raw(1, cal.raw, 3, 1), us_b, vs_b, valid_b, fill=-1.0)
  assert np.isfinite(out).all() and (out[:, :, ~valid_b] == -1.0).all()


@pytest.mark.parametrize("shape", [s for s in rr.SHAPES if s[7]], ids=[s[0] for s in rr.SHAPES if s[7]])
def test_the_out_of_bounds_shapes_run_both_branches(shape):
  case = rr.shape_case(shape)
  for m in case["map"]:
    assert 0.2 <= m[2].mean() <= 0.8


def test_shapes_place_the_kernels_constants():
  widths = {s[6][3] for s in rr.SHAPES}
  assert {1, 3, 5, rr.RC_SPAN - 1, rr.RC_SPAN, rr.RC_SPAN + 1} <= widths
  assert {w % 4 for w in widths} == {0, 1, 2, 3}
  assert {1, 2, rr.RC_ROWS + 1} <= {s[6][2] for s in rr.SHAPES}
  assert {s[3] for s in rr.SHAPES} == {1, 3} and {s[4] for s in rr.SHAPES} == {1, 3}
  assert any(s[6][0] % 2 and s[6][1] % 2 for s in rr.SHAPES)
  assert any(s[5][0] < s[6][2] and s[5][1] < s[6][3] for s in rr.SHAPES) and any(s[5][1] == 1 for s in rr.SHAPES)


def test_identity_calibration_is_a_crop():
  src = rr.random_raw(2, (9, 14), 3, 3)
  out = rr.rectify(rr.IDENTITY, src, (2, 3, 5, 7))
  want = np.moveaxis(src[:, 2:7, 3:10].astype(F) / F(255), 3, 1)
  assert np.array_equal(rr.bits(out), rr.bits(want))


# ------------------------------------------------------------------------------------------------------------ geometry
def _rig():
  cam_l = rx.RawCamera(rr.KITTI_LIKE.K_matrix(), rr.KITTI_LIKE.D[:5], (512, 1392))
  cam_r = rx.RawCamera(rr.KITTI_LIKE_R.K_matrix(), rr.KITTI_LIKE_R.D[:5], (512, 1392))
  R = rx.rodrigues(np.array([0.011, -0.023, 0.007]))
  T = np.array([-0.5371, 0.0042, -0.0093])
  return cam_l, cam_r, R, T


def test_geometry_through_the_fp64_map():
  cam_l, cam_r, R, T = _rig()
  R1, R2, P1, P2 = rx.stereo_rectify(cam_l, cam_r, R, T, new_size=(375, 1242))
  for Rc in (R1, R2):
    assert np.abs(Rc.dot(Rc.T) - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Rc) - 1) < 1e-14
  f = min(cam_l.K[1, 1], cam_r.K[1, 1])
  assert P1[0, 0] == f and P1[1, 1] == f and P1[0, 3] == 0 and np.array_equal(P1[:, :3], P2[:, :3])
  assert abs(P2[0, 3] + f * np.linalg.norm(T)) <= 1e-8 and P2[1, 3] == 0
  view_l, view_r = rx.RectifiedView(cam_l, R1, P1, (375, 1242)), rx.RectifiedView(cam_r, R2, P2, (375, 1242))

  rng = np.random.RandomState(7)
  z = rng.uniform(4.0, 60.0, 500)
  X_l = np.stack([rng.uniform(-0.45, 0.45, 500) * z, rng.uniform(-0.14, 0.14, 500) * z, z], axis=1)
  X_r = X_l.dot(R.T) + T
  rect_l, rect_r = view_l.project(X_l), view_r.project(X_r)
  assert np.abs(rect_l[:, 1] - rect_r[:, 1]).max() <= 1e-8                      # the two rectified rows agree
  via_p2 = X_l.dot(R1.T).dot(P2[:, :3].T) + P2[:, 3]                            # P2 . [R1 x; 1]: the left rectified frame into the right view
  assert np.abs(via_p2[:, :2] / via_p2[:, 2:] - rect_r).max() <= 1e-8
  disp = rect_l[:, 0] - rect_r[:, 0]
  depth = X_l.dot(R1.T)[:, 2]
  assert np.abs(disp - f * np.linalg.norm(T) / depth).max() <= 1e-8            # disparity = f * b / z of the rectified frame
  for view, cam, X, rect in ((view_l, cam_l, X_l, rect_l), (view_r, cam_r, X_r, rect_r)):
    us, vs, valid = rr.coords(view_calib(view), cam.size, rect[:, 0], rect[:, 1], np.float64)
    raw = cam.project(X)
    assert np.abs(us - raw[:, 0]).max() <= 1e-8 and np.abs(vs - raw[:, 1]).max() <= 1e-8    # the map returns the raw pixel
    assert valid.mean() > 0.5
  # a point at infinity: the same pixel in both views
  d = rng.uniform(-0.3, 0.3, (50, 3))
  d[:, 2] = 1.0
  p_l = d.dot(R1.T).dot(P1[:, :3].T)
  p_r = d.dot(R.T).dot(R2.T).dot(P2[:, :3].T)
  assert np.abs(p_l[:, :2] / p_l[:, 2:] - p_r[:, :2] / p_r[:, 2:]).max() <= 1e-8


def test_stereo_rectify_of_an_ideal_rig_is_the_identity():
  cam = rx.RawCamera(rr.KITTI_LIKE.K_matrix(), [0, 0, 0, 0], (512, 1392))
  R1, R2, P1, P2 = rx.stereo_rectify(cam, cam, np.eye(3), [-0.54, 0.0, 0.0])
  assert np.array_equal(R1, np.eye(3)) and np.array_equal(R2, np.eye(3))
  assert P1[0, 0] == cam.K[1, 1] and abs(P2[0, 3] + 0.54 * cam.K[1, 1]) <= 1e-12
  # the centre of the raw image lands on the centre of the new one
  assert abs(P1[0, 2] - ((1392 - 1) / 2.0 - P1[0, 0] * ((1392 - 1) / 2.0 - cam.K[0, 2]) / cam.K[0, 0])) <= 1e-9
  assert rx.stereo_camera(rx.RectifiedView(cam, R1, P1), rx.RectifiedView(cam, R2, P2)).baseline == pytest.approx(0.54, abs=1e-12)


def test_rodrigues_round_trip():
  for v in ([0.3, -0.2, 0.5], [0.0, 0.0, 0.0], [1e-9, 0.0, 0.0], [0.0, 2.5, 0.0]):
    R = rx.rodrigues(np.array(v))
    assert np.abs(R.dot(R.T) - np.eye(3)).max() < 1e-14
    assert np.abs(rx.rodrigues(R) - np.array(v)).max() < 1e-12
  assert np.abs(rx.rodrigues(np.array([0.008, -0.012, 0.004])) - rr.KITTI_R).max() < 1e-15


def _write_calib(path, pairs):
  fmt = lambda a: " ".join("%.6e" % v for v in np.asarray(a, dtype=np.float64).reshape(-1))
  with open(path, "w") as f:
    f.write("calib_time: 09-Jan-2012 13:57:47\ncorner_dist: 9.950000e-02\n")
    for c, cal in pairs:
      f.write("S_0%d: %s\n" % (c, fmt([cal.raw[1], cal.raw[0]])))
      f.write("K_0%d: %s\n" % (c, fmt(cal.K_matrix())))
      f.write("D_0%d: %s\n" % (c, fmt(cal.D[:5])))
      f.write("R_0%d: %s\nT_0%d: %s\n" % (c, fmt(np.eye(3)), c, fmt(np.zeros(3))))
      f.write("S_rect_0%d: %s\n" % (c, fmt([cal.window[3], cal.window[2]])))
      f.write("R_rect_0%d: %s\n" % (c, fmt(cal.R)))
      f.write("P_rect_0%d: %s\n" % (c, fmt(cal.P_matrix())))


def test_kitti_raw_rectification_from_file(tmp_path):
  path = str(tmp_path / "calib_cam_to_cam.txt")
  _write_calib(path, [(0, rr.RATIONAL), (2, rr.KITTI_LIKE), (3, rr.KITTI_LIKE_R)])
  calib = rx.KittiRawRectification.from_file(path)
  assert calib.raw_size == (512, 1392) and calib.rect_size == (375, 1242)
  for view, cal in ((calib.view_l, rr.KITTI_LIKE), (calib.view_r, rr.KITTI_LIKE_R)):
    assert np.allclose(view.raw.K, cal.K_matrix(), rtol=1e-6, atol=0) and np.allclose(view.raw.D, cal.D, rtol=1e-6, atol=0)
    assert np.allclose(view.R, cal.R, atol=1e-6) and np.allclose(view.P, cal.P_matrix(), rtol=1e-6, atol=0)
    assert view.raw.D[5:].tolist() == [0, 0, 0]
    # the struct the kernel gets: the restatement's constants, each rounded once
    nat_cam, (m, K, D) = view.native(), view_calib(view).constants(F)
    assert [F(v) for v in nat_cam.m] == list(m)
    assert (F(nat_cam.fx), F(nat_cam.fy), F(nat_cam.cx), F(nat_cam.cy)) == K
    assert tuple(F(getattr(nat_cam, n)) for n in ("k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6")) == D
  cam = calib.camera
  assert cam.baseline == pytest.approx(0.5327, abs=5e-5)
  assert (cam.fx, cam.cx, cam.cy) == pytest.approx((721.5377, 609.5593, 172.854), rel=1e-6)
  with pytest.raises(ValueError, match="differ in size"):
    rx.KittiRawRectification.from_file(path, cams=(0, 3))
  with pytest.raises(ValueError, match="K_01"):
    rx.KittiRawRectification.from_file(path, cams=(1, 3))


def test_argument_errors_of_the_host_classes():
  K = rr.KITTI_LIKE.K_matrix()
  with pytest.raises(ValueError, match="4, 5 or 8"):
    rx.RawCamera(K, [0.1] * 6, (512, 1392))
  with pytest.raises(ValueError, match="K must be"):
    rx.RawCamera(np.eye(3) * 2, [0.0] * 4, (512, 1392))
  with pytest.raises(ValueError, match="finite 3x3"):
    rx.RawCamera(np.zeros((3, 4)), [0.0] * 4, (512, 1392))
  with pytest.raises(ValueError, match="size"):
    rx.RawCamera(K, [0.0] * 4, (0, 1392))
  cam = rx.RawCamera(K, [0.0] * 5, (512, 1392))
  P = rr.KITTI_LIKE.P_matrix()
  with pytest.raises(ValueError, match="not a rotation"):
    rx.RectifiedView(cam, np.eye(3) * 1.01, P)
  with pytest.raises(ValueError, match="P_rect must be"):
    rx.RectifiedView(cam, np.eye(3), np.ones((3, 4)))
  with pytest.raises(ValueError, match="RawCamera"):
    rx.RectifiedView(K, np.eye(3), P)
  with pytest.raises(ValueError, match="horizontal rig"):
    rx.stereo_rectify(cam, cam, np.eye(3), [0.0, -0.5, 0.0])            # a vertical rig
  with pytest.raises(ValueError, match="horizontal rig"):
    rx.stereo_rectify(cam, cam, np.eye(3), [0.5, 0.0, 0.0])             # the first camera on the right
  with pytest.raises(ValueError, match="not a rotation"):
    rx.stereo_rectify(cam, cam, np.eye(3) * 2, [-0.5, 0.0, 0.0])
  view_l, view_r = calib_view(rr.KITTI_LIKE), calib_view(rr.KITTI_LIKE_R)
  other = rr.KITTI_LIKE_R.P_matrix()
  other[0, 2] += 1.0
  with pytest.raises(ValueError, match="share fx, fy, cx and cy"):
    rx.Rectifier(view_l, rx.RectifiedView(view_r.raw, view_r.R, other, view_r.size), (512, 1392))
  with pytest.raises(ValueError, match="on the right"):
    rx.Rectifier(view_r, view_l, (512, 1392))
  with pytest.raises(ValueError, match="window"):
    rx.Rectifier(view_l, view_r, (512, 1392), window=(0, 0, 0, 5))
  with pytest.raises(ValueError, match="channels"):
    rx.Rectifier(view_l, view_r, (512, 1392), channels=2)
  with pytest.raises(RuntimeError, match="no CPU path"):
    rx.Rectifier(view_l, view_r, (512, 1392), device="cpu")
