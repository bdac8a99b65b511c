"""tests/pointcloud_ref.py — the host restatement that tests/test_gpu_pointcloud.py compares csrc/pointcloud.hip against bit for
bit — held to things that do not depend on it: torch's bilinear down-sampling, a scene small enough to work by hand, and the
all-float64 physics of depth = fx * b / disp."""
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointcloud_ref as pr
from conftest import parity_note


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("H,W", [(10, 13), (37, 131), (75, 259)])
def test_downsample_is_torch_bilinear_within_2_ulp(H, W, s):
  """m = ((a + b) + (c + d)) * 0.25f is F.interpolate(scale_factor=1/n, bilinear, align_corners=False), the node's line 145, up
  to the order of torch's four products: within 2 ulp, not always bit-equal — the written definition is the contract."""
  x = torch.rand(2, 1, H, W, generator=torch.Generator().manual_seed(H * 1000 + W + s)) * 190
  want = F.interpolate(x, scale_factor=1.0 / 2 ** s, mode="bilinear", align_corners=False).numpy()
  got = pr.downsample(x.numpy(), s)
  assert got.shape == want.shape == (2, 1, H >> s, W >> s)
  ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
  worst = float(np.max(np.abs(got.astype(np.float64) - want) / ulp))
  parity_note("pointcloud_downsample_vs_torch_%dx%d_s%d" % (H, W, s), worst_ulp=worst,
              bit_equal_share=float(np.mean(got == want)))
  assert worst <= 2.0


def test_six_pixel_scene_worked_by_hand():
  """2 x 3 pixels at s = 0, fx = fy = 2, baseline 3 (fb = 6), cx = 1, cy = -0.5, voxel 4 m:
       (0,0) disp 1/16 -> depth 96  -> z = 96 > depth_trunc          invalid
       (0,1) disp 1.5  -> z = 4: x = 0,  y = 1      voxel ( 0,0,1)   colour (255,127,  0)
       (0,2) disp 1    -> z = 6: x = 3,  y = 1.5    voxel ( 0,0,1)   colour (127,127, 63)
       (1,0) disp 1    -> z = 6: x = -3, y = 4.5    voxel (-1,1,1)   colour ( 63,255,191)   floor(-0.75) = -1
       (1,1) disp 1.5  -> z = 4: x = 0,  y = 3      voxel ( 0,0,1)   colour (  0,191, 63)
       (1,2) disp 0    -> depth inf -> 100 -> z = 100 > depth_trunc  invalid
     voxel (0,0,1): three points, mean (1, 5.5/3, 14/3), colour (382 // 3, 445 // 3, 126 // 3) = (127, 148, 42)."""
  disp = np.array([[[[1 / 16, 1.5, 1.0], [1.0, 1.5, 0.0]]]], np.float32)
  rgb = np.zeros((1, 3, 2, 3), np.float32)
  rgb[0, :, 0, 1] = (1.0, 0.5, 0.0)
  rgb[0, :, 0, 2] = (0.5, 0.5, 0.25)
  rgb[0, :, 1, 0] = (0.25, 1.0, 0.75)
  rgb[0, :, 1, 1] = (0.0, 0.75, 0.25)
  rgb[0, :, 0, 0] = rgb[0, :, 1, 2] = 1.0                  # invalid pixels: their colour must not reach any voxel
  cam = pr.camera_constants(2.0, 2.0, 1.0, -0.5, 3.0, 0)
  p = pr.points(disp, cam, 0)
  assert p["depth"][0].tolist() == [[96.0, 4.0, 6.0], [6.0, 4.0, 100.0]]
  assert p["q"][0].tolist() == [[9600, 400, 600], [600, 400, 10000]]
  assert p["valid"][0].tolist() == [[False, True, True], [True, True, False]]
  org = pr.organized(p)
  assert np.isnan(org[0, :, 0, 0]).all() and np.isnan(org[0, :, 1, 2]).all()
  assert org[0, :, 1, 0].tolist() == [-3.0, 4.5, 6.0]
  cloud = pr.voxel_cloud(p, 0, 4.0, pr.colour_bytes(rgb, 0))
  assert cloud["n"] == 2 and cloud["dropped"] == 0
  assert cloud["voxel"].tolist() == [[-1, 1, 1], [0, 0, 1]]
  assert cloud["count"].tolist() == [1, 3]
  want = struct.pack("<fffI", -3.0, 4.5, 6.0, (63 << 16) | (255 << 8) | 191) + \
         struct.pack("<fffI", 1.0, 5.5 / 3, 14.0 / 3, (127 << 16) | (148 << 8) | 42)
  assert pr.record_bytes(cloud) == want
  # without colour the fourth word is 0
  plain = pr.voxel_cloud(p, 0, 4.0)
  assert pr.record_bytes(plain) == struct.pack("<fffI", -3.0, 4.5, 6.0, 0) + struct.pack("<fffI", 1.0, 5.5 / 3, 14.0 / 3, 0)
  # quantisation off: z is the depth itself, (0,0) and (1,2) stay beyond depth_trunc
  p0 = pr.points(disp, cam, 0, depth_scale=0.0)
  assert p0["valid"][0].tolist() == [[False, True, True], [True, True, False]] and p0["z"][0, 0, 1] == 4.0


def test_index_range_and_nan_pixels():
  """|i| >= 2^20 is dropped, not inserted; a NaN disparity is invalid and counted nowhere."""
  disp = np.array([[[[1.0, 1.0, float("nan"), -1.0]]]], np.float32)
  cam = pr.camera_constants(1e-4, 1.0, 2.0, 0.0, 1e4, 0)          # fb = 1: z = 1; x = (u - 2) / 1e-4 = -20000, -10000
  p = pr.points(disp, cam, 0)
  assert p["valid"][0, 0].tolist() == [True, True, False, False]
  assert np.isnan(p["depth"][0, 0, 2]) and p["depth"][0, 0, 3] == 0.0
  cloud = pr.voxel_cloud(p, 0, 0.015)                             # -20000 / 0.015 = -1.33e6: out; -10000 / 0.015 = -6.7e5: in
  assert cloud["n"] == 1 and cloud["dropped"] == 1 and cloud["voxel"][0, 0] == -666667


def test_fp32_quantum_against_fp64_physics():
  """q = (int)(depth * depth_scale) from the fp32 definition against all-float64 arithmetic on a 4 x 375 x 1242 frame at s = 2
  (disparities uniform in [0, 190), fx * b = 1329 * 0.54): the two may disagree only where depth * depth_scale sits within
  fp32 rounding of an integer — by exactly one quantum, at no more than 1e-3 of the pixels (the definition alone gives a
  few in 1e5: the cap has room, and a wrong operation order or a dropped rounding cannot hide under it)."""
  g = torch.Generator().manual_seed(20211)
  disp = (torch.rand(4, 1, 375, 1242, generator=g) * 190).numpy()
  fx, fy, cx, cy, b = 1329.0, 1329.0, 617.3, 181.6, 0.54
  p = pr.points(disp, pr.camera_constants(fx, fy, cx, cy, b, 2), 2)
  ph = pr.physics(disp, fx, fy, cx, cy, b, 2)
  assert p["q"].shape == (4, 93, 310)
  diff = np.abs(p["q"] - ph["q"])
  share = float(np.mean(diff != 0))
  parity_note("pointcloud_q_fp32_vs_fp64", pixels=int(diff.size), differing=int(np.sum(diff != 0)), share=share,
              largest=int(diff.max()))
  assert diff.max() <= 1
  assert share <= 1e-3
  # where the quantum agrees the back-projection agrees to fp32 precision: five roundings relative to x (z, fxs, the
  # difference, the product, the quotient) and the rounding of cxs, which the difference u - cxs does not shrink
  same = (diff == 0) & p["valid"]
  eps = 2.0 ** -24
  for k, c, f in (("x", cx / 4, fx / 4), ("y", cy / 4, fy / 4)):
    err = np.abs(p[k].astype(np.float64) - ph[k])
    bound = 5 * eps * np.abs(ph[k]) + eps * abs(c) * ph["z"] / f
    assert bool(np.all(err[same] <= bound[same])), float(np.max(err[same] / bound[same]))


def test_camera_from_dataset_and_constructor_refusals():
  """StereoCamera.from_dataset scales the intrinsics a StereoDataset records; a data set without them raises there.  The
  projector's argument checks come before anything touches a GPU."""
  from adaptive_stereo.datasets.stereo_dataset import StereoDataset
  from adaptive_stereo.pointcloud import DepthProjector, StereoCamera
  ds = StereoDataset.__new__(StereoDataset)           # the calibration methods need the data set's name only
  ds.dataset = "KittiRaw"
  cam = StereoCamera.from_dataset(ds, 375, 1242)
  K = ds.get_intrinsics(375, 1242)
  assert (cam.fx, cam.fy, cam.cx, cam.cy, cam.baseline) == (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), 0.54)
  assert abs(cam.fx - 0.5885 * 1242) < 1e-3
  c = cam.native(2, 100.0, 100.0, 80.0)
  want = pr.camera_constants(cam.fx, cam.fy, cam.cx, cam.cy, cam.baseline, 2)
  assert all(np.float32(getattr(c, k)) == want[k] for k in want)                  # rounded once, to the same fp32 values
  ds.dataset = "VirtualKitti"
  with pytest.raises(NotImplementedError):
    StereoCamera.from_dataset(ds, 375, 1242)
  with pytest.raises(ValueError, match="65535"):
    DepthProjector(375, 1242, cam, max_depth=656.0)
  with pytest.raises(ValueError, match="power of two"):
    DepthProjector(375, 1242, cam, table_slots=3000)
  with pytest.raises(ValueError, match="pyramid_scale"):
    DepthProjector(375, 1242, cam, pyramid_scale=3)
