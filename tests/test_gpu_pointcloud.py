"""adaptive_stereo.pointcloud (csrc/pointcloud.hip) against tests/pointcloud_ref.py, BIT FOR BIT: depth, the organised cloud and
its NaN pattern, and for voxel clouds the set of voxels, their counts, means, packed colours, n and dropped, after sorting both
sides by (ix, iy, iz) — the order of records within an image is the only thing the contract leaves open.  A NaN depth (NaN
disparity) is compared by position, every other word by its bits.

What the cases are for:
  per-pixel   ragged sizes at every pyramid scale, a row width (131) that ends rows mid-wave, more than one workgroup; planted
              disparities 0, 1e-30, negative, NaN, and values that put depth * depth_scale within an ulp or two of an integer on
              either side, and depth just across max_depth and depth_trunc; the same with quantisation off.
  voxel       many points per voxel (contention, long runs of equal keys in a wave), one point per voxel, negative indices;
              with colour and without; a table filled to 96 % and one of exactly h*w slots (long probe chains, wrap-around);
              indices beyond 2^20 (dropped, never inserted); a second frame and a graph replay that must not see the first.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from adaptive_stereo import _native as nat
from adaptive_stereo.pointcloud import DepthProjector, StereoCamera, VoxelCloud
import pointcloud_ref as pr

DEV = "cuda:0"
F = np.float32


def _camera(H, W, fx=721.5, baseline=0.54):
  return StereoCamera(fx, fx * 1.03, 0.37 * W + 0.3, 0.45 * H + 0.7, baseline)      # centre non-integer and off-centre


def _consts(cam, s):
  return pr.camera_constants(cam.fx, cam.fy, cam.cx, cam.cy, cam.baseline, s)


def _steps(x, j):
  x = F(x)
  for _ in range(abs(j)):
    x = np.nextafter(x, F(np.inf) if j > 0 else F(-np.inf), dtype=F)
  return x


def _planted(fb):
  """disparities at the decision edges: depth * 100 around the integers 577 and 1234, depth around depth_trunc = 80 and
  max_depth = 100, each at -2 .. +2 ulp of the disparity that lands nearest; then 0, 1e-30, a negative and a NaN"""
  vals = [F(0), F(1e-30), F(-3), F(np.nan)]
  for k in (8000, 10000, 577, 1234):
    m0 = F(fb) / (F(k) / F(100))
    vals += [_steps(m0, j) for j in (-2, -1, 0, 1, 2)]
  return vals


def _plant(disp, s, values, seed):
  """every value at its own output pixel (all source taps of that pixel: the 2x2 mean of four equal values is the value)"""
  B, _, H, W = disp.shape
  n = 1 << s
  h, w = H >> s, W >> s
  o = n // 2 - 1 if s else 0
  values = values[:max(4, (B * h * w) // 2)]
  at = np.random.RandomState(seed).permutation(B * h * w)[:len(values)]
  for val, i in zip(values, at):
    b, v, u = i // (h * w), (i % (h * w)) // w, i % w
    disp[b, 0, n * v + o:n * v + o + (2 if s else 1), n * u + o:n * u + o + (2 if s else 1)] = val
  return disp


def _random_disp(B, H, W, seed, lo=0.5, hi=190.0):
  return (lo + (hi - lo) * np.random.RandomState(seed).rand(B, 1, H, W)).astype(F)


def _image(B, H, W, seed):
  return np.random.RandomState(seed).rand(B, 3, H, W).astype(F)


def _bits(a):
  return np.ascontiguousarray(a, dtype=F).view(np.int32)


def _same_bits_or_nan(got, want, what):
  assert got.shape == want.shape, what
  gn, wn = np.isnan(got), np.isnan(want)
  assert np.array_equal(gn, wn), "%s: NaN pattern differs at %d pixels" % (what, int(np.sum(gn != wn)))
  bad = (_bits(got) != _bits(want)) & ~wn
  assert not bad.any(), "%s: %d of %d words differ, first %r" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist())


def _check_cloud(cloud, disp, cam, s, voxel_size, rgb=None, expect_dropped=0, **depth_args):
  """every image of a VoxelCloud against the reference; returns the reference clouds"""
  assert isinstance(cloud, VoxelCloud)
  p = pr.points(disp, _consts(cam, s), s, **depth_args)
  colour = None if rgb is None else pr.colour_bytes(rgb, s)
  got = cloud.trim()
  refs = []
  for b in range(disp.shape[0]):
    ref = pr.voxel_cloud(p, b, voxel_size, colour)
    g = got[b]
    assert int(cloud.n[b]) == ref["n"] == g["voxel"].shape[0], "image %d: %d voxels, reference %d" % (b, int(cloud.n[b]), ref["n"])
    assert g["dropped"] == ref["dropped"], "image %d: dropped %d, reference %d" % (b, g["dropped"], ref["dropped"])
    if expect_dropped is not None:
      assert g["dropped"] == expect_dropped
    vox, cnt, rec = pr.sort_cloud(g["voxel"].cpu().numpy(), g["count"].cpu().numpy(), g["records"].cpu().numpy())
    assert np.array_equal(vox, ref["voxel"]), "image %d: voxel sets differ" % b
    assert np.array_equal(cnt, ref["count"]), "image %d: counts differ" % b
    assert np.array_equal(rec[:, :3], _bits(ref["xyz"])), "image %d: %d mean words differ" % (
        b, int(np.sum(rec[:, :3] != _bits(ref["xyz"]))))
    assert np.array_equal(rec[:, 3].view(np.uint32), ref["rgb"]), "image %d: packed colours differ" % b
    assert np.array_equal(_bits(g["xyz"].cpu().numpy()), g["records"].cpu().numpy()[:, :3])     # .xyz is the float view
    refs.append(ref)
  return refs


# ---- 1. per-pixel stage -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth_scale", [100.0, 0.0])
@pytest.mark.parametrize("B,H,W,s", [(2, 10, 13, 2), (1, 37, 131, 1), (2, 75, 259, 0), (2, 75, 259, 2), (1, 23, 524, 2)])
def test_depth_and_organized_cloud_bit_exact(B, H, W, s, depth_scale):
  cam = _camera(H, W)
  disp = _plant(_random_disp(B, H, W, seed=H * W + s), s, _planted(_consts(cam, s)["fb"]), seed=s + 1)
  proj = DepthProjector(H, W, cam, batch=B, pyramid_scale=s, depth_scale=depth_scale, device=DEV)
  xyz, depth = proj.organized(torch.from_numpy(disp).to(DEV))
  assert tuple(xyz.shape) == (B, 3, H >> s, W >> s) and tuple(depth.shape) == (B, 1, H >> s, W >> s)
  xyz, depth = xyz.cpu().numpy(), depth.cpu().numpy()
  p = pr.points(disp, _consts(cam, s), s, depth_scale=depth_scale)
  if B * (H >> s) * (W >> s) >= 48:                       # the planted edges are all there, and they do decide something
    assert np.isnan(p["depth"]).sum() == 1 and (p["depth"] == 0).sum() == 1 and (p["depth"] == 100).sum() >= 4
    assert 0 < (~p["valid"]).sum() < p["valid"].size
  _same_bits_or_nan(depth[:, 0], p["depth"], "depth")
  want = pr.organized(p)
  assert np.array_equal(_bits(xyz), _bits(want)), "organised cloud: %d of %d words differ (NaN pattern: %d)" % (
      int(np.sum(_bits(xyz) != _bits(want))), want.size, int(np.sum(np.isnan(xyz) != np.isnan(want))))
  # depth() alone writes the same map
  depth2 = proj.depth(torch.from_numpy(disp).to(DEV)).cpu().numpy()
  _same_bits_or_nan(depth2[:, 0], p["depth"], "depth()")


# ---- 2. voxel clouds ----------------------------------------------------------------------------------------------------------
def _scene(name, B, H, W, s, cam):
  """(disp, voxel_size)"""
  rs = np.random.RandomState(len(name) + H)
  if name == "near_plane":          # fronto-parallel at ~2.6 m: a handful of voxels take hundreds of points each
    return (150.0 + 0.5 * rs.rand(B, 1, H, W)).astype(F), (0.5 if s else 0.15)
  if name == "far_ramp":            # 20 .. 70 m, neighbouring pixels >= 2.7 cm apart in x: at 1 mm every point owns its voxel
    ramp = np.linspace(cam.fx * cam.baseline / 20.0, cam.fx * cam.baseline / 70.0, W, dtype=F)
    return np.broadcast_to(ramp, (B, 1, H, W)).copy() * (1 + 0.01 * rs.rand(B, 1, H, W)).astype(F), 0.001
  assert name == "random"           # depth log-uniform from 2 m to 195 m (a fifth beyond depth_trunc), on both sides of x = 0 and y = 0;
  n = 1 << s                        # constant over each output pixel's block, so that the 2x2 mean keeps the spread
  coarse = np.exp(rs.uniform(np.log(2.0), np.log(190.0), (B, 1, H // n + 1, W // n + 1)))
  return np.kron(coarse, np.ones((n, n)))[:, :, :H, :W].astype(F), 0.15


@pytest.mark.parametrize("colour", [True, False])
@pytest.mark.parametrize("name,B,H,W,s", [("near_plane", 2, 23, 524, 2), ("far_ramp", 2, 23, 524, 2), ("random", 2, 23, 524, 2),
                                          ("near_plane", 1, 75, 259, 0)])
def test_voxel_cloud_bit_exact(name, B, H, W, s, colour):
  cam = _camera(H, W)
  disp, voxel_size = _scene(name, B, H, W, s, cam)
  rgb = _image(B, H, W, seed=5) if colour else None
  proj = DepthProjector(H, W, cam, batch=B, pyramid_scale=s, voxel_size=voxel_size, device=DEV)
  cloud = proj.voxel_cloud(torch.from_numpy(disp).to(DEV), None if rgb is None else torch.from_numpy(rgb).to(DEV))
  refs = _check_cloud(cloud, disp, cam, s, voxel_size, rgb)
  points = (H >> s) * (W >> s)
  for ref in refs:                                          # the scenes are what their names say
    if name == "near_plane":
      assert ref["count"].sum() == points and ref["n"] <= 40 and ref["count"].max() >= 100
    elif name == "far_ramp":
      assert ref["n"] == ref["count"].sum() == points
    else:
      assert (ref["voxel"][:, 0] < 0).any() and (ref["voxel"][:, 0] > 0).any()
      assert (ref["voxel"][:, 1] < 0).any() and (ref["voxel"][:, 1] > 0).any() and ref["count"].sum() < points
  if not colour:
    assert int(cloud.records[..., 3].abs().max()) == 0


# ---- 3. nearly full table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,slots", [(1, 60, 68, 256), (2, 23, 524, 1024), (1, 64, 64, 256)])
def test_nearly_full_table(B, H, W, slots):
  """15 x 17 = 255 pixels, 245 of them valid and each in a voxel of its own, in 256 slots; 655 in 1024 = the power of two above
  h*w; 256 in 256: probe chains as long as the table and wrapping round its end, and still nothing dropped."""
  s = 2
  cam = _camera(H, W)
  disp, voxel_size = _scene("far_ramp", B, H, W, s, cam)
  h, w = H >> s, W >> s
  if (H, W) == (60, 68):
    _plant(disp, s, [F(0)] * 10, seed=3)                   # depth 100 > depth_trunc: ten invalid pixels
  assert slots >= h * w and slots < 2 * h * w
  proj = DepthProjector(H, W, cam, batch=B, pyramid_scale=s, voxel_size=voxel_size, device=DEV, table_slots=slots)
  cloud = proj.voxel_cloud(torch.from_numpy(disp).to(DEV))
  refs = _check_cloud(cloud, disp, cam, s, voxel_size)
  for ref in refs:
    assert ref["n"] == (245 if (H, W) == (60, 68) else h * w)


# ---- 4. index range -----------------------------------------------------------------------------------------------------------
def test_indices_beyond_2_pow_20_are_dropped_not_inserted():
  B, H, W, s = 2, 23, 524, 2
  cam = StereoCamera(0.005, 721.5, 0.37 * W + 0.3, 0.45 * H + 0.7, 0.54 * 721.5 / 0.005)   # fxs = 0.00125: x up to ~5e6 m
  disp = _random_disp(B, H, W, seed=9, lo=4.0, hi=190.0)
  proj = DepthProjector(H, W, cam, batch=B, pyramid_scale=s, device=DEV)
  cloud = proj.voxel_cloud(torch.from_numpy(disp).to(DEV))
  refs = _check_cloud(cloud, disp, cam, s, 0.15, expect_dropped=None)
  for ref in refs:
    assert ref["dropped"] >= 50 and ref["n"] >= 50 and np.abs(ref["voxel"]).max() < 2 ** 20
    assert np.abs(ref["voxel"][:, 0]).max() > 2 ** 19       # the kept ones reach far into the range


# ---- 5. independence and capture ----------------------------------------------------------------------------------------------
def test_second_frame_sees_nothing_of_the_first():
  B, H, W, s = 2, 23, 524, 2
  cam = _camera(H, W)
  proj = DepthProjector(H, W, cam, batch=B, pyramid_scale=s, device=DEV)
  rgb = _image(B, H, W, seed=6)
  for name in ("random", "near_plane", "random"):
    disp, _ = _scene(name, B, H, W, s, cam)
    cloud = proj.voxel_cloud(torch.from_numpy(disp).to(DEV), torch.from_numpy(rgb).to(DEV))
    _check_cloud(cloud, disp, cam, s, 0.15, rgb)
  # a smaller batch through the same buffers
  disp, _ = _scene("random", 1, H, W, s, cam)
  _check_cloud(proj.voxel_cloud(torch.from_numpy(disp).to(DEV)), disp, cam, s, 0.15)


def test_captured_graph_replays_with_new_contents():
  B, H, W, s = 2, 23, 524, 2
  cam = _camera(H, W)
  proj = DepthProjector(H, W, cam, batch=B, pyramid_scale=s, device=DEV)
  first, _ = _scene("near_plane", B, H, W, s, cam)
  second, _ = _scene("random", B, H, W, s, cam)
  rgb = _image(B, H, W, seed=8)
  static_disp, static_rgb = torch.from_numpy(first).to(DEV), torch.from_numpy(rgb).to(DEV)
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    proj.voxel_cloud(static_disp, static_rgb)               # warm-up outside the capture
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):     # one stream: a linear graph
    cloud = proj.voxel_cloud(static_disp, static_rgb)       # allocates nothing, synchronises nothing: capturable
  graph.replay()
  torch.cuda.synchronize()
  _check_cloud(cloud, first, cam, s, 0.15, rgb)
  static_disp.copy_(torch.from_numpy(second))
  graph.replay()
  torch.cuda.synchronize()
  _check_cloud(cloud, second, cam, s, 0.15, rgb)


# ---- 6. from the model --------------------------------------------------------------------------------------------------------
def test_cloud_from_the_models_disparity(golden_loader):
  from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
  from adaptive_stereo.utils import synthetic as syn
  meta = golden_loader("crop_96x256_k4_b1").meta
  fnet = FeatureExtractorNetwork(meta["k"])
  snet = StereoNet(meta["k"], 1, meta["s"], maxdisp=meta["maxdisp"])
  fnet.load_state_dict(syn.synthetic_state_dict(fnet.state_dict(), seed=123), strict=True)
  snet.load_state_dict(syn.synthetic_state_dict(snet.state_dict(), seed=123, logit_gain=meta["gain"]), strict=True)
  fnet, snet = fnet.to(DEV).eval(), snet.to(DEV).eval()
  left, right = (t.to(DEV) for t in syn.stereo_pair(meta["B"], meta["H"], meta["W"], seed=1))
  with torch.no_grad():
    out = snet(left, fnet(left), fnet(right), "l")
  disp = out["pred_disp_l/0"].detach().contiguous()
  H, W = meta["H"], meta["W"]
  assert tuple(disp.shape) == (1, 1, H, W)
  cam = StereoCamera(0.5885 * W, 1.9501 * H, 0.4972 * W, 0.4972 * H, 0.54)          # the KITTI intrinsics the data set records
  proj = DepthProjector(H, W, cam, batch=1, pyramid_scale=2, device=DEV)
  cloud = proj.voxel_cloud(disp, left.contiguous())
  host_disp, host_left = disp.cpu().numpy(), left.cpu().numpy()
  (ref,) = _check_cloud(cloud, host_disp, cam, 2, 0.15, host_left)
  assert ref["n"] >= 20                                                              # a cloud, not an empty frame
  data = cloud.to_pointcloud2_bytes(0)
  assert len(data) == 16 * ref["n"]
  rec = np.frombuffer(data, dtype=pr.RECORD)
  order = np.lexsort((rec["z"], rec["y"], rec["x"]))
  want = np.frombuffer(pr.record_bytes(ref), dtype=pr.RECORD)
  assert rec[order].tobytes() == want[np.lexsort((want["z"], want["y"], want["x"]))].tobytes()


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------
def test_errors_are_raised_before_anything_is_launched():
  H, W = 23, 524
  cam = _camera(H, W)
  with pytest.raises(ValueError, match="65535"):
    DepthProjector(H, W, cam, max_depth=700.0, depth_scale=100.0, device=DEV)
  with pytest.raises(ValueError, match="power of two"):
    DepthProjector(H, W, cam, device=DEV, table_slots=1000)
  with pytest.raises(ValueError, match="power of two"):
    DepthProjector(H, W, cam, device=DEV, table_slots=512)              # < h*w = 655
  proj = DepthProjector(H, W, cam, batch=1, device=DEV)
  disp = torch.from_numpy(_random_disp(1, H, W, seed=1)).to(DEV)
  cloud = proj.voxel_cloud(disp)
  torch.cuda.synchronize()
  before = [t.clone() for t in (cloud.records, cloud.voxel, cloud.count, cloud.n, cloud.dropped, proj._depth, proj._xyz)]
  with pytest.raises(RuntimeError, match="no CPU path"):
    proj.voxel_cloud(disp.cpu())
  with pytest.raises(RuntimeError, match="no CPU path"):
    proj.voxel_cloud(disp, torch.zeros(1, 3, H, W))
  with pytest.raises(RuntimeError, match=r"\(1, 1, 23, 520\)"):
    proj.depth(disp[..., :520].contiguous())
  with pytest.raises(RuntimeError, match=r"\(1, 3, 22, 524\)"):
    proj.voxel_cloud(disp, torch.zeros(1, 3, 22, W, device=DEV))
  with pytest.raises(RuntimeError, match="at most 1"):
    proj.organized(torch.cat([disp, disp]))
  # the C ABI validates before it launches, too
  lib = nat.load()
  c = cam.native(2, 700.0, 100.0, 80.0)
  import ctypes
  assert lib.as_disp_to_points(nat.ptr(disp), None, 1, H, W, 2, ctypes.byref(c), nat.ptr(proj._depth), None, 0.15, None, 0,
                               nat.stream()) != 0
  assert b"16-bit" in lib.as_last_error()
  c = cam.native(2, 100.0, 100.0, 80.0)
  assert lib.as_disp_to_points(nat.ptr(disp), None, 1, H, W, 2, ctypes.byref(c), None, None, 0.15, nat.ptr(proj._table), 512,
                               nat.stream()) != 0
  assert b"slots" in lib.as_last_error()
  assert lib.as_voxel_table_slots(655) == 2048 and lib.as_voxel_table_slots(10) == 1024 and lib.as_voxel_table_slots(512) == 1024
  torch.cuda.synchronize()
  after = (cloud.records, cloud.voxel, cloud.count, cloud.n, cloud.dropped, proj._depth, proj._xyz)
  assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, after))    # nothing ran
  # and the projector still works: the table was left clean
  _check_cloud(proj.voxel_cloud(disp), disp.cpu().numpy(), cam, 2, 0.15)
