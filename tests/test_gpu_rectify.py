"""csrc/rectify.hip (as_rectify_map, as_rectify_pair) and adaptive_stereo.rectify on the GPU, bit for bit against the float32
restatement of tests/rectify_ref.py (pinned against float64 and against the camera model on the CPU by
tests/test_rectify_ref_cpu.py).  Every output is written between sentinel guards, as tests/test_gpu_disp_filter.py does.

The frame kernel's workgroup covers RC_ROWS = 4 rows x RC_SPAN = 256 columns, 4 pixels per lane (64 columns apart);
rectify_ref.SHAPES places its boundaries by these, and keeps W % 4 in {0, 1, 2, 3} and outputs off 16-byte alignment, where a
kernel with wider stores would have to take another route."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rectify_ref as rr
from test_gpu_end_to_end import build
from test_rectify_ref_cpu import _write_calib, calib_view
from adaptive_stereo import _native as nat
from adaptive_stereo import consistency as cons
from adaptive_stereo import disp_filter as dfm
from adaptive_stereo import rectify as rx
from adaptive_stereo.pointcloud import DepthProjector

DEV = "cuda:0"
F = np.float32
SENTINEL = -7777.0
GUARD = 64
NET_B, NET_H, NET_W, NET_K, NET_MAXDISP = 2, 83, 150, 3, 100          # the small network and shapes of tests/test_gpu_both_view.py
NET_RAW, NET_WINDOW = (128, 348), (5, 81, NET_H, NET_W)


def native_cam(cal):
  """the struct from the restatement's own constants (not through adaptive_stereo.rectify)"""
  m, K, D = cal.constants(F)
  cam = nat.RectifyCamera()
  cam.m[:] = [float(v) for v in m]
  cam.fx, cam.fy, cam.cx, cam.cy = [float(v) for v in K]
  cam.k1, cam.k2, cam.p1, cam.p2, cam.k3, cam.k4, cam.k5, cam.k6 = [float(v) for v in D]
  return cam


class Guarded(object):
  """one fp32 buffer of n elements inside a sentinel-filled allocation, GUARD elements on either side; `shift` elements of
  extra offset take the buffer off the 16-byte alignment of the allocation"""

  def __init__(self, n, shift=0):
    self.raw = torch.full((n + 2 * GUARD + shift,), SENTINEL, dtype=torch.float32, device=DEV)
    self.view = self.raw[GUARD + shift:GUARD + shift + n]
    self.lo, self.hi = GUARD + shift, GUARD + shift + n

  def guards_intact(self):
    return bool((self.raw[:self.lo] == SENTINEL).all()) and bool((self.raw[self.hi:] == SENTINEL).all())

  def untouched(self):
    return bool((self.raw == SENTINEL).all())


def same_bits(got, want):
  got = got.cpu().numpy()
  assert got.shape == want.shape and got.dtype == want.dtype == F, (got.shape, want.shape, got.dtype, want.dtype)
  return np.array_equal(got.view(np.uint32), want.view(np.uint32))


def assert_same(got, want, what):
  if not same_bits(got, want):
    g = got.cpu().numpy()
    bad = np.argwhere(g.view(np.uint32) != want.view(np.uint32))
    raise AssertionError("%s: %d of %d elements differ, first %s: got %r, want %r"
                         % (what, len(bad), g.size, bad[:4].tolist(), g[tuple(bad[0])], want[tuple(bad[0])]))
  return True


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_map(cal, raw, window, which=("map_x", "map_y", "valid")):
  i0, j0, H, W = window
  g = {k: Guarded(H * W) for k in ("map_x", "map_y", "valid")}
  nat.call("as_rectify_map", native_cam(cal), raw[0], raw[1], i0, j0, H, W,
           *([nat.ptr(g[k].view) if k in which else None for k in ("map_x", "map_y", "valid")] + [nat.stream()]))
  torch.cuda.synchronize()
  for k, b in g.items():
    assert b.guards_intact(), "a write outside %s" % k
    if k not in which:
      assert b.untouched(), "%s was not requested and was written" % k
  return {k: g[k].view.reshape(H, W) for k in which}


def run_pair(case, fill=None, shift=0):
  """as_rectify_pair on one entry of rectify_ref.shape_case -> (left, right) device tensors [B,3,H,W]"""
  B, C, (H0, W0), (i0, j0, H, W) = case["B"], case["C"], case["raw"], case["window"]
  g = [Guarded(B * 3 * H * W, shift), Guarded(B * 3 * H * W, shift)]
  src = [dev(s) for s in case["src"]]
  nat.call("as_rectify_pair", nat.ptr(src[0]), nat.ptr(src[1]), B, H0, W0, C, native_cam(case["cal"][0]), native_cam(case["cal"][1]),
           i0, j0, H, W, case["fill"] if fill is None else fill, nat.ptr(g[0].view), nat.ptr(g[1].view), nat.stream())
  torch.cuda.synchronize()
  for b, side in zip(g, ("left", "right")):
    assert b.guards_intact(), "a write outside the %s output" % side
  return [b.view.reshape(B, 3, H, W) for b in g]


@pytest.fixture(scope="module")
def cases():
  """the inputs and the restatement's answers of every shape, computed once and left unchanged"""
  return {s[0]: rr.shape_case(s, fill=0.0 if i % 2 else 0.375) for i, s in enumerate(rr.SHAPES)}


# ====================================================================================================== as_rectify_map
@pytest.mark.parametrize("name", rr.SHAPE_IDS)
def test_map_bit_equal(cases, name):
  case = cases[name]
  for side in (0, 1):
    got = run_map(case["cal"][side], case["raw"], case["window"])
    us, vs, valid = case["map"][side]
    assert_same(got["map_x"], us, "%s map_x[%d]" % (name, side))              # NaN and infinities included: the bits
    assert_same(got["map_y"], vs, "%s map_y[%d]" % (name, side))
    assert_same(got["valid"], valid.astype(F), "%s valid[%d]" % (name, side))
    if case["oob"]:
      assert 0.2 <= valid.mean() <= 0.8                                        # both branches run


def test_map_every_null_combination(cases):
  case = cases["horizon"]
  want = dict(zip(("map_x", "map_y", "valid"), case["map"][1]))
  want["valid"] = want["valid"].astype(F)
  for which in (("map_x",), ("map_y",), ("valid",), ("map_x", "map_y"), ("map_x", "valid"), ("map_y", "valid")):
    got = run_map(case["cal"][1], case["raw"], case["window"], which)
    for k in which:
      assert_same(got[k], want[k], "%s of %s" % (k, which))


def test_map_full_kitti_window_is_all_valid():
  cal = rr.KITTI_LIKE
  got = run_map(cal, cal.raw, cal.window)
  us, vs, valid = rr.rectify_map(cal, cal.raw, cal.window)
  assert valid.all()
  assert_same(got["map_x"], us, "map_x") and assert_same(got["map_y"], vs, "map_y")
  assert bool((got["valid"] == 1.0).all())


# ===================================================================================================== as_rectify_pair
@pytest.mark.parametrize("name", rr.SHAPE_IDS)
def test_pair_bit_equal(cases, name):
  case = cases[name]
  got = run_pair(case)
  for side in (0, 1):
    assert_same(got[side], case["dst"][side], "%s %s" % (name, ("left", "right")[side]))
    valid = case["map"][side][2]
    if case["oob"]:
      assert 0.2 <= valid.mean() <= 0.8
    assert bool((got[side].cpu().numpy()[:, :, ~valid] == F(case["fill"])).all())


@pytest.mark.parametrize("name", ["span", "right_wide", "horizon_mono_wide"])
def test_pair_on_outputs_that_are_not_16_byte_aligned(cases, name):
  """the outputs need 4-byte alignment only: the shapes with W % 4 == 0 at offsets of 4 and 8 bytes, the same bits"""
  case = cases[name]
  assert case["window"][3] % 4 == 0
  for shift in (1, 2):
    got = run_pair(case, shift=shift)
    assert got[0].data_ptr() % 16 != 0
    for side in (0, 1):
      assert_same(got[side], case["dst"][side], "%s shifted by %d, side %d" % (name, shift, side))


@pytest.mark.parametrize("name", ["span-2", "horizon", "top_wide_mono"])
def test_pair_samples_at_the_maps_coordinates(cases, name):
  """one coordinate function: the reference's sampler fed with what as_rectify_map REPORTED gives what as_rectify_pair wrote"""
  case = cases[name]
  got = run_pair(case)
  for side in (0, 1):
    m = run_map(case["cal"][side], case["raw"], case["window"])
    us, vs, valid = [m[k].cpu().numpy() for k in ("map_x", "map_y", "valid")]
    want = rr.sample(case["src"][side], us, vs, valid == 1.0, case["fill"])
    assert_same(got[side], want, "%s side %d" % (name, side))


def test_pair_left_and_right_are_not_swapped_and_fill_is_used(cases):
  case = cases["left"]                                           # one calibration for both sides, two different images
  assert not np.array_equal(case["src"][0], case["src"][1])
  other = dict(case, cal=(rr.QUARTER, rr.RATIONAL))
  other["map"] = tuple(rr.rectify_map(c, case["raw"], case["window"]) for c in other["cal"])
  for fill in (-1.5, float("inf")):
    other["dst"] = tuple(rr.sample(s, m[0], m[1], m[2], fill) for s, m in zip(other["src"], other["map"]))
    got = run_pair(other, fill=fill)
    assert_same(got[0], other["dst"][0], "left") and assert_same(got[1], other["dst"][1], "right")
    assert not np.array_equal(other["dst"][0], other["dst"][1])
    assert bool((got[0].cpu().numpy()[:, :, ~other["map"][0][2]] == F(fill)).all())
  # the cameras swapped give the swapped result: each source is read with its own camera
  swapped = dict(other, cal=other["cal"][::-1], src=other["src"][::-1])
  got = run_pair(swapped, fill=float("inf"))
  assert_same(got[0], other["dst"][1], "swapped left") and assert_same(got[1], other["dst"][0], "swapped right")


def test_identity_calibration_equals_decode_rgb8():
  B, H0, W0, window = 2, 21, 70, (3, 5, 17, 64)
  src = rr.random_raw(B, (H0, W0), 3, 21)
  case = dict(B=B, C=3, raw=(H0, W0), window=window, cal=(rr.IDENTITY, rr.IDENTITY), src=(src, src[::-1].copy()), fill=0.0)
  for win in (window, (3, 5, 17, 63)):                           # W % 4 == 0 and not
    case["window"] = win
    got = run_pair(case)
    i0, j0, H, W = win
    for side in (0, 1):
      s = dev(case["src"][side])
      want = torch.full((B, 3, H, W), SENTINEL, dtype=torch.float32, device=DEV)
      for b in range(B):
        nat.call("as_decode_rgb8", nat.ptr(s[b]), H0, W0, i0, j0, H, W, 0, nat.ptr(want[b]), nat.stream())
      torch.cuda.synchronize()
      assert torch.equal(got[side].view(torch.int32), want.view(torch.int32))


def test_bad_arguments_return_err_arg_and_leave_the_outputs_untouched(cases):
  case = cases["w3"]
  B, C, (H0, W0), (i0, j0, H, W) = case["B"], case["C"], case["raw"], case["window"]
  src = dev(case["src"][0])
  cam = native_cam(case["cal"][0])
  out = [Guarded(B * 3 * H * W), Guarded(B * 3 * H * W)]
  lib = nat.load()
  good = dict(src_l=nat.ptr(src), src_r=nat.ptr(src), B=B, H0=H0, W0=W0, C=C, cam_l=cam, cam_r=cam, i0=i0, j0=j0, H=H, W=W, fill=0.0,
              dst_l=nat.ptr(out[0].view), dst_r=nat.ptr(out[1].view), stream=nat.stream())
  bad = [("src_l", None), ("src_r", None), ("cam_l", None), ("cam_r", None), ("dst_l", None), ("dst_r", None), ("B", 0), ("B", -1),
         ("B", 32768), ("H0", 0), ("W0", 0), ("C", 2), ("C", 4), ("C", 0), ("H", 0), ("W", 0), ("H", -3), ("i0", 2 ** 30 + 1),
         ("j0", -2 ** 30 - 1), ("dst_l", nat.c_vp(out[0].view.data_ptr() + 2))]
  for key, value in bad:
    args = dict(good)
    args[key] = value
    assert lib.as_rectify_pair(*args.values()) == -1, (key, value)
    assert lib.as_last_error().decode().startswith("as_rectify_pair:")
  torch.cuda.synchronize()
  assert out[0].untouched() and out[1].untouched()
  assert lib.as_rectify_pair(*good.values()) == 0
  torch.cuda.synchronize()
  assert not out[0].untouched() and out[0].guards_intact()

  m = [Guarded(H * W) for _ in range(3)]
  good = dict(cam=cam, H0=H0, W0=W0, i0=i0, j0=j0, H=H, W=W, map_x=nat.ptr(m[0].view), map_y=nat.ptr(m[1].view), valid=nat.ptr(m[2].view),
              stream=nat.stream())
  for key, value in [("cam", None), ("H0", 0), ("W0", -1), ("H", 0), ("W", 0), ("i0", -2 ** 30 - 1), ("j0", 2 ** 30 + 1)]:
    args = dict(good)
    args[key] = value
    assert lib.as_rectify_map(*args.values()) == -1, (key, value)
  args = dict(good, map_x=None, map_y=None, valid=None)
  assert lib.as_rectify_map(*args.values()) == -1 and "no output" in lib.as_last_error().decode()
  torch.cuda.synchronize()
  assert all(b.untouched() for b in m)


# =========================================================================================================== Rectifier
def test_rectifier_outputs_camera_and_foreign_buffer():
  view_l, view_r = calib_view(rr.QUARTER), calib_view(rr.QUARTER_R)
  window = (-19, -61, 40, 130)                                   # leaves the raw image at the top and on the left
  rect = rx.Rectifier(view_l, view_r, (128, 348), window=window, batch=2, fill=0.5, device=DEV)
  src = [rr.random_raw(2, (128, 348), 3, seed) for seed in (31, 32)]
  want = [rr.rectify(cal, s, window, fill=0.5) for cal, s in zip((rr.QUARTER, rr.QUARTER_R), src)]
  left, right = rect(dev(src[0]), dev(src[1]))
  assert_same(left, want[0], "left") and assert_same(right, want[1], "right")
  maps = [rr.rectify_map(cal, (128, 348), window) for cal in (rr.QUARTER, rr.QUARTER_R)]
  (mxl, myl), (mxr, myr) = rect.maps()
  assert_same(mxl, maps[0][0], "map_x_l") and assert_same(myr, maps[1][1], "map_y_r")
  assert_same(mxr, maps[1][0], "map_x_r") and assert_same(myl, maps[0][1], "map_y_l")
  for v, m in ((rect.valid_l, maps[0]), (rect.valid_r, maps[1])):
    assert tuple(v.shape) == (2, 1, 40, 130) and v.is_contiguous()
    assert_same(v, np.broadcast_to(m[2].astype(F), (2, 1, 40, 130)).copy(), "valid")
  fl, fr = rect.valid_fraction()
  assert fl == pytest.approx(maps[0][2].mean(), abs=1e-6) and fr == pytest.approx(maps[1][2].mean(), abs=1e-6)
  assert 0.2 < fl < 0.8
  cam = rect.camera
  f, cx, cy = rr.QUARTER.P
  assert (cam.fx, cam.fy, cam.cx, cam.cy) == (f, f, cx + 61, cy + 19)
  assert cam.baseline == pytest.approx((44.857 + 339.52) / 721.5377, rel=1e-12)
  # out=: a foreign buffer, e.g. the two halves of one allocation
  pair = Guarded(2 * 2 * 3 * 40 * 130)
  halves = pair.view.reshape(2, 2, 3, 40, 130)
  before = left.clone()
  l2, r2 = rect(dev(src[1]), dev(src[0]), out=(halves[0], halves[1]))
  torch.cuda.synchronize()
  assert l2.data_ptr() == halves[0].data_ptr() and pair.guards_intact()
  assert_same(l2, rr.rectify(rr.QUARTER, src[1], window, fill=0.5), "out= left")
  assert_same(r2, rr.rectify(rr.QUARTER_R, src[0], window, fill=0.5), "out= right")
  assert torch.equal(left, before)                               # the rectifier's own buffers were not written
  # valid_l gates a cloud as any confidence map does
  proj = DepthProjector(40, 130, cam, batch=2, pyramid_scale=0)
  disp = torch.full((2, 1, 40, 130), 20.0, device=DEV)
  cloud = proj.voxel_cloud(disp, l2, confidence=rect.valid_l, conf_min=1.0)
  torch.cuda.synchronize()
  assert cloud.rejected.cpu().tolist() == [int((~maps[0][2]).sum())] * 2
  with pytest.raises(RuntimeError, match="no CPU path"):
    rect(torch.from_numpy(src[0]), dev(src[1]))
  with pytest.raises(RuntimeError, match="contiguous uint8"):
    rect(dev(src[0])[:, :, :, :1], dev(src[1]))
  with pytest.raises(RuntimeError, match="out\\[1\\] must be"):
    rect(dev(src[0]), dev(src[1]), out=(halves[0], halves[1][:, :, :-1].contiguous()))
  mono = rx.Rectifier(view_l, view_r, (128, 348), window=(3, 5, 6, 9), channels=1, device=DEV)
  ml, _ = mono(dev(src[0][:1, :, :, :1]), dev(src[1][:1, :, :, :1]))
  assert_same(ml, rr.rectify(rr.QUARTER, src[0][:1, :, :, :1], (3, 5, 6, 9)), "mono")


# ================================================================================================== RectifiedInference
@pytest.fixture(scope="module")
def world():
  fnet, snet = build(dict(k=NET_K, s=0, maxdisp=NET_MAXDISP, gain=200.0))
  fnet.eval(); snet.eval()
  frames = [(dev(rr.random_raw(NET_B, NET_RAW, 3, 40 + 2 * i)), dev(rr.random_raw(NET_B, NET_RAW, 3, 41 + 2 * i))) for i in range(2)]
  return dict(fnet=fnet, snet=snet, frames=frames)


def _flat(result):
  out = []
  for item in result:
    out.extend(t for t in item if t is not None) if isinstance(item, tuple) else out.append(item)
  return [t.clone() for t in out]


def _same(a, b, what):
  assert len(a) == len(b)
  for i, (x, y) in enumerate(zip(a, b)):
    assert x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), "%s: output %d differs" % (what, i)
  return True


def test_rectified_inference_with_the_identity_calibration_equals_inner_on_decoded_images(world):
  ident = rr.Calib(rr.IDENTITY.K, rr.IDENTITY.D, rr.IDENTITY.R, rr.IDENTITY.P, 0.0, NET_RAW, (0, 0) + NET_RAW)
  right = rr.Calib(ident.K, ident.D, ident.R, ident.P, -0.5, NET_RAW, (0, 0) + NET_RAW)
  rect = rx.Rectifier(calib_view(ident), calib_view(right), NET_RAW, window=NET_WINDOW, batch=NET_B, device=DEV)
  assert rect.valid_fraction() == (1.0, 1.0)
  raw_l, raw_r = world["frames"][0]
  decoded = torch.empty(2, NET_B, 3, NET_H, NET_W, device=DEV)
  for side, raw in enumerate((raw_l, raw_r)):
    for b in range(NET_B):
      nat.call("as_decode_rgb8", nat.ptr(raw[b]), NET_RAW[0], NET_RAW[1], NET_WINDOW[0], NET_WINDOW[1], NET_H, NET_W, 0,
               nat.ptr(decoded[side, b]), nat.stream())
  want = _flat(cons.BothViewInference(world["fnet"], world["snet"], NET_H, NET_W, batch=NET_B)(decoded[0], decoded[1]))
  chain = rx.RectifiedInference(cons.BothViewInference(world["fnet"], world["snet"], NET_H, NET_W, batch=NET_B), rect)
  got = _flat(chain(raw_l, raw_r))
  torch.cuda.synchronize()
  _same(got, want, "identity")
  assert float(want[0].std()) > 0


@pytest.mark.parametrize("filtered", [False, True], ids=["both_view", "filtered"])
def test_rectified_inference_eager_replayed_and_overwritten_inputs(world, filtered):
  make = (lambda: dfm.FilteredBothViewInference(world["fnet"], world["snet"], NET_H, NET_W, batch=NET_B)) if filtered else \
         (lambda: cons.BothViewInference(world["fnet"], world["snet"], NET_H, NET_W, batch=NET_B))
  rect = rx.Rectifier(calib_view(rr.QUARTER), calib_view(rr.QUARTER_R), NET_RAW, window=NET_WINDOW, batch=NET_B, device=DEV)
  assert rect.valid_fraction() == (1.0, 1.0)
  (l0, r0), (l1, r1) = world["frames"]
  # inner alone, on the Rectifier's output
  want = []
  for l, r in ((l0, r0), (l1, r1)):
    left, right = rect(l, r)
    assert_same(left, rr.rectify(rr.QUARTER, l.cpu().numpy(), NET_WINDOW), "rectified left")
    want.append(_flat(make()(left.clone(), right.clone())))
  assert not torch.equal(want[0][0], want[1][0])                 # two different frames
  chain = rx.RectifiedInference(make(), rect)
  assert len(chain(l0, r0)) == (5 if filtered else 4)
  eager = []
  for l, r in ((l0, r0), (l1, r1)):
    l, r = l.clone(), r.clone()
    res = chain(l, r)
    l.fill_(0); r.fill_(255)                                     # the raw inputs may be overwritten after the call
    eager.append(_flat(res))
  torch.cuda.synchronize()
  _same(eager[0], want[0], "eager frame 0") and _same(eager[1], want[1], "eager frame 1")

  outer, side, x = torch.cuda.CUDAGraph(), torch.cuda.Stream(), torch.zeros(4, device=DEV)
  torch.cuda.synchronize()
  with torch.cuda.graph(outer, stream=side, capture_error_mode="thread_local"):
    x.add_(1.0)
    with pytest.raises(RuntimeError, match="already being captured"):
      chain.capture()
  assert chain.capture(l0, r0) is chain
  for i, (l, r) in enumerate(((l1, r1), (l0, r0))):
    l, r = l.clone(), r.clone()
    res = chain(l, r)                                            # two copies of raw bytes + one replay
    l.fill_(7); r.fill_(9)
    torch.cuda.synchronize()
    _same(_flat(res), want[1 - i], "replayed frame %d" % (1 - i))
  with pytest.raises(RuntimeError, match="contiguous uint8"):
    chain(l0[:, :-1].contiguous(), r0)
  with pytest.raises(ValueError, match="the rectifier produces"):
    rx.RectifiedInference(cons.BothViewInference(world["fnet"], world["snet"], NET_H, NET_W + 1, batch=NET_B), rect)


# ====================================================================================================== rectify_raw.py
def test_rectify_raw_cli_writes_the_reference_rounded(tmp_path, capsys):
  from PIL import Image
  import rectify_raw
  raw, rect_size = (64, 174), (47, 155)
  cal_l = rr.KITTI_LIKE.scaled(0.125, raw, (0, 0) + rect_size)
  cal_r = rr.KITTI_LIKE_R.scaled(0.125, raw, (0, 0) + rect_size)
  calib = str(tmp_path / "calib_cam_to_cam.txt")
  _write_calib(calib, [(2, cal_l), (3, cal_r)])
  for side in ("image_02", "image_03"):
    os.makedirs(str(tmp_path / side))
  src = {}
  for k, name in enumerate(("0000000000.png", "0000000007.png")):
    for side, seed in (("image_02", 50 + k), ("image_03", 60 + k)):
      src[side, name] = rr.random_raw(1, raw, 3, seed)
      Image.fromarray(src[side, name][0]).save(str(tmp_path / side / name))
  n, rect = rectify_raw.rectify_raw(str(tmp_path / "image_02"), str(tmp_path / "image_03"), calib, str(tmp_path / "out"), fill=0.25)
  assert n == 2 and (rect.H, rect.W) == rect_size
  text = capsys.readouterr().out
  view = rx.KittiRawRectification.from_file(calib)              # the file's 7 digits, not the calibration's own
  assert "fx {:.6f} fy {:.6f} cx {:.6f} cy {:.6f}".format(view.camera.fx, view.camera.fy, view.camera.cx, view.camera.cy) in text
  assert "Baseline: {:.6f} m".format(view.camera.baseline) in text
  assert view.camera.baseline == pytest.approx(0.125 * (44.857 + 339.52) / (0.125 * 721.5377), rel=1e-5)
  from test_rectify_ref_cpu import view_calib
  for side, out_side, v in (("image_02", "left", view.view_l), ("image_03", "right", view.view_r)):
    cal = view_calib(v, raw, (0, 0) + rect_size)
    for name in ("0000000000.png", "0000000007.png"):
      got = np.asarray(Image.open(str(tmp_path / "out" / out_side / name)))
      ref = rr.rectify(cal, src[side, name], (0, 0) + rect_size, fill=0.25)[0]
      want = np.clip(np.floor(ref * F(255) + F(0.5)), 0, 255).astype(np.uint8).transpose(1, 2, 0)
      assert got.shape == want.shape and np.array_equal(got, want), (side, name, int((got != want).sum()))
