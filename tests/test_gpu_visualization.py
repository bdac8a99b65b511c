"""csrc/visualize.hip (as_colormap_range, as_colormap_apply, as_image_to_cv) and adaptive_stereo/utils/visualization.py on the GPU.

References, none of them the kernels under test: the reference's own outputs (tests/golden/visualization.npz, written by
tests/golden/make_golden_visualization.py) and tests/visualization_ref.py, which tests/test_visualization_ref_cpu.py holds to that
fixture bit for bit.  Every comparison is exact: the outputs are table entries selected by a contract of single IEEE operations.
"""
import csv
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import visualization_ref as R
from adaptive_stereo import _native as nat
from adaptive_stereo.utils import visualization as V
from conftest import GOLDEN_DIR

DEV = "cuda:0"
GUARD = 16
SENTINEL = 0xA5
CASES = [(shape, config) for shape in R.SHAPES for config in R.configs_for(shape)]
IDS = [R.case_name(s, c) for s, c in CASES]
MODE_DTYPE = {0: torch.uint8, 1: torch.uint8, 2: torch.float32, 3: torch.int16}


@pytest.fixture(scope="module")
def fixture():
  return np.load(os.path.join(GOLDEN_DIR, "visualization.npz"), allow_pickle=False)


def same(a, b):
  a, b = np.asarray(a), np.asarray(b)
  return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def guarded(shape, dtype):
  """(whole buffer, view of `shape`): 16 sentinel bytes in front of the view and 16 behind its LAST BYTE, wherever that falls."""
  n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
  buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
  return buf, buf[GUARD:GUARD + n].view(dtype).view(shape)


def guards_untouched(buf):
  return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def device_tables(table):
  return {0: torch.from_numpy(V.table_u8(table)).to(DEV), 1: torch.from_numpy(V.table_u8(table)).to(DEV),
          2: torch.from_numpy(table.astype(np.float32)).to(DEV), 3: None}


def run(x, table, vmin, vmax, mode, y=None, n=None):
  """The C entry points themselves on device tensors -> numpy output of `mode`, guards checked."""
  B, _, H, W = x.shape
  n = table.shape[0] - 3 if n is None else n
  shape = {0: (B, H, W, 3), 1: (B, H, W, 3), 2: (B, 3, H, W), 3: (B, H, W)}[mode]
  buf, out = guarded(shape, MODE_DTYPE[mode])
  automatic, lo, hi, den = V._bounds(vmin, vmax)
  ws = torch.full((nat.load().as_colormap_workspace(B, H * W) // 4,), float("nan"), device=DEV)
  if automatic:
    nat.call("as_colormap_range", nat.ptr(x), nat.ptr(y), B, H, W, nat.ptr(ws), nat.stream())
  nat.call("as_colormap_apply", nat.ptr(x), nat.ptr(y), B, H, W, automatic, lo, hi, den, nat.ptr(ws) if automatic else None,
           nat.ptr(device_tables(table)[mode]), n, mode, nat.ptr(out), nat.stream())
  torch.cuda.synchronize()
  assert guards_untouched(buf), "mode %d wrote outside its output" % mode
  return out.cpu().numpy()


@pytest.mark.parametrize("shape,config", CASES, ids=IDS)
def test_every_case_and_mode_against_the_reference(fixture, shape, config):
  kind, vmin, vmax, cmap = config
  name = R.case_name(shape, config)
  x_host = R.make_case(shape, kind)
  assert np.array_equal(R.checksum(x_host), fixture["check__" + name])
  x = torch.from_numpy(x_host).to(DEV)
  table = fixture["table__" + cmap]
  want_u8 = fixture["u8__" + name]
  assert same(run(x, table, vmin, vmax, 1), want_u8), "u8 BGR"
  assert same(run(x, table, vmin, vmax, 0), np.ascontiguousarray(want_u8[..., ::-1])), "u8 RGB"
  idx = run(x, table, vmin, vmax, 3)
  assert same(idx, R.index(x_host, vmin, vmax)), "index"
  f = run(x, table, vmin, vmax, 2)
  assert same(f, R.paint_f32(table, idx)), "f32"
  if R.stores_float(shape, config):
    assert same(f, fixture["f32__" + name]), "f32 against the reference"
    assert same(table[idx.astype(np.int64)], fixture["rgba__" + name]), "apply_cmap against the reference"


@pytest.mark.parametrize("vmin,vmax", [(None, None), (0, R.R115)], ids=["auto", "fixed"])
def test_kitti_size_against_the_restatement(fixture, vmin, vmax):
  x_host = R.make_case(R.KITTI, "nan" if vmin is not None else "plain")
  x = torch.from_numpy(x_host).to(DEV)
  table = fixture["table__inferno"]
  idx = R.index(x_host, vmin, vmax)
  assert len(np.unique(idx)) > 200
  assert same(run(x, table, vmin, vmax, 3), idx)
  assert same(run(x, table, vmin, vmax, 1), R.paint_u8(table, idx, "bgr"))
  assert same(run(x, table, vmin, vmax, 2), R.paint_f32(table, idx))


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "b%d_h%d_w%d" % (s[0], s[2], s[3]))
def test_mixed_bounds_against_the_restatement(fixture, shape):
  kind, vmin, vmax, cmap = R.MIXED
  x_host = R.make_case(shape, kind)
  x = torch.from_numpy(x_host).to(DEV)
  table = fixture["table__" + cmap]
  for lo, hi in ((vmin, vmax), (None, 80)):
    idx = R.index(x_host, lo, hi)
    assert same(run(x, table, lo, hi, 3), idx)
    assert same(run(x, table, lo, hi, 1), R.paint_u8(table, idx, "bgr"))


def test_many_small_images_and_an_unaligned_input(fixture):
  """40 images of 5x5: one workgroup spans all of them, so most pixels fold their image's partials themselves.  Then the same
  map read from an address that is 4- but not 16-byte aligned (the scalar loads)."""
  table = fixture["table__magma"]
  x_host = R.make_case((40, 1, 5, 5), "plain")
  x_host[7, 0, 2, 2] = np.float32("nan")
  x = torch.from_numpy(x_host).to(DEV)
  idx = R.index(x_host, None, None)
  assert (idx[7] == 258).all() and (idx[8] != 258).all()
  assert same(run(x, table, None, None, 3), idx)
  assert same(run(x, table, None, None, 0), R.paint_u8(table, idx, "rgb"))
  flat = torch.zeros(x.numel() + 1, device=DEV)
  flat[1:] = x.reshape(-1)
  shifted = flat[1:].view(x.shape)
  assert shifted.data_ptr() % 16 == 4
  for vmin, vmax in ((None, None), (0, 80)):
    assert same(run(shifted, table, vmin, vmax, 1), run(x, table, vmin, vmax, 1))


def test_paint_error_is_the_map_of_the_absolute_difference(fixture):
  shape = R.SHAPES[2]
  pred_host, gt_host = R.make_case(shape, "plain"), R.make_case(shape, "edges80")
  pred, gt = torch.from_numpy(pred_host).to(DEV), torch.from_numpy(gt_host).to(DEV)
  err = (gt - pred).abs()
  table = fixture["table__hot"]
  for vmin, vmax in ((None, None), (0, 80)):
    want = run(err, table, vmin, vmax, 1)
    assert same(run(pred, table, vmin, vmax, 1, y=gt), want)
    assert same(want, R.paint_u8(table, R.index(pred_host, vmin, vmax, y=gt_host), "bgr"))
    painter = V.DisparityPainter(shape[2], shape[3], batch=2, cmap="hot", vmin=vmin, vmax=vmax, device=DEV)
    assert same(painter.paint_error(pred, gt).cpu().numpy(), want)
    assert same(painter.paint(err).cpu().numpy(), want)


def test_a_table_of_ten_entries(fixture):
  """N < 256: the duck-typed colour map of tests/visualization_ref.py, through the painter."""
  TenSteps = R.TenSteps
  shape = R.SHAPES[2]
  x_host = R.make_case(shape, "infs")
  x_host[1, 0, 0, 0] = np.float32("nan")
  table, n = V.colormap_table(TenSteps())
  idx = R.index(x_host, 0, 80, N=10)
  assert set(np.unique(idx)) == set(range(13))
  x = torch.from_numpy(x_host).to(DEV)
  for out, want in (("u8", R.paint_u8(table, idx, "rgb")), ("f32", R.paint_f32(table, idx)), ("index", idx)):
    painter = V.DisparityPainter(shape[2], shape[3], batch=2, cmap=TenSteps(), vmin=0, vmax=80, order="rgb", out=out, device=DEV)
    assert same(painter.paint(x).cpu().numpy(), want), out


def test_conversions_against_the_reference(fixture):
  for hw in R.CONVERSION_SHAPES:
    tag = "%dx%d" % hw
    rgb, gray, disp = R.make_image(3, hw), R.make_image(1, hw), R.make_disp_image(hw)
    for put in (lambda a: torch.from_numpy(a).to(DEV), torch.from_numpy):       # device tensors, then CPU tensors
      if "cv_rgb__" + tag in fixture.files:
        assert same(V.tensor_to_cv_rgb(put(rgb)), fixture["cv_rgb__" + tag])
      assert same(V.tensor_to_cv_rgb(put(np.ascontiguousarray(np.moveaxis(rgb, 0, -1)))), fixture["cv_rgb_last__" + tag])
      assert same(V.tensor_to_cv_gray(put(gray)), fixture["cv_gray__" + tag])
      assert same(V.tensor_to_cv_disp(put(disp)), fixture["cv_disp__" + tag])
      assert same(V.tensor_to_cv_disp(put(disp), cast_uint8=False), fixture["cv_disp_f32__" + tag])
      assert same(V.tensor_to_cv_disp(put(disp)[0]), fixture["cv_disp_2d__" + tag])
  # the C entry point with guards: 3 x 37 x 53 bytes is no dword multiple; two images; saturation
  hw = R.CONVERSION_SHAPES[2]
  imgs = np.stack([R.make_image(3, hw), R.make_image(3, hw, seed=1)])
  imgs[1, :, 0, :4] = np.array([-0.5, 1.5, np.nan, np.inf], np.float32)
  x = torch.from_numpy(imgs).to(DEV)
  buf, out = guarded((2,) + hw + (3,), torch.uint8)
  nat.call("as_image_to_cv", nat.ptr(x), 2, 3, hw[0], hw[1], 1, 0.0, 0, nat.ptr(out), nat.stream())
  torch.cuda.synchronize()
  assert guards_untouched(buf)
  assert same(out.cpu().numpy(), np.stack([R.to_cv_rgb(imgs[0]), R.to_cv_rgb(imgs[1])]))
  assert out[1, 0, :4, 0].tolist() == [0, 255, 0, 255]
  painter = V.DisparityPainter(hw[0], hw[1], batch=2, order="bgr", device=DEV)
  assert same(painter.rgb(x).cpu().numpy(), out.cpu().numpy())
  painter = V.DisparityPainter(hw[0], hw[1], batch=2, order="rgb", device=DEV)
  assert same(painter.rgb(x).cpu().numpy(), out.cpu().numpy()[..., ::-1].copy())


def test_error_returns(fixture):
  lib = nat.load()
  x = torch.zeros(1, 1, 4, 4, device=DEV)
  table = torch.from_numpy(V.table_u8(fixture["table__magma"])).to(DEV)
  buf, out = guarded((1, 4, 4, 3), torch.uint8)
  ws = torch.zeros(64, device=DEV)
  st = nat.stream()

  def apply(xp=nat.ptr(x), B=1, H=4, W=4, automatic=0, wsp=None, tp=nat.ptr(table), N=256, mode=1, outp=nat.ptr(out)):
    return lib.as_colormap_apply(xp, None, B, H, W, automatic, 0.0, 0.0, 1.0, wsp, tp, N, mode, outp, st)

  assert apply() == 0
  for kwargs, text in ((dict(xp=None), b"NULL"), (dict(outp=None), b"NULL"), (dict(tp=None), b"table"), (dict(B=0), b"positive"),
                       (dict(H=0), b"positive"), (dict(W=-1), b"positive"), (dict(N=0), b"N 0"), (dict(N=257), b"N 257"),
                       (dict(mode=4), b"mode"), (dict(automatic=3), b"workspace"), (dict(automatic=4), b"automatic"),
                       (dict(outp=nat.c_vp(out.data_ptr() + 1)), b"aligned"), (dict(outp=nat.c_vp(out.data_ptr() + 2)), b"aligned")):
    assert apply(**kwargs) != 0, kwargs
    assert text in lib.as_last_error(), (kwargs, lib.as_last_error())
  assert apply(mode=3, tp=None) == 0                                 # the index needs no table
  assert lib.as_colormap_range(None, None, 1, 4, 4, nat.ptr(ws), st) != 0
  assert lib.as_colormap_range(nat.ptr(x), None, 1, 4, 4, None, st) != 0
  assert lib.as_colormap_range(nat.ptr(x), None, 1, 0, 4, nat.ptr(ws), st) != 0
  assert lib.as_colormap_workspace(0, 16) < 0 and lib.as_colormap_workspace(1, 0) < 0 and lib.as_colormap_workspace(2, 1 << 30) < 0
  assert lib.as_colormap_workspace(2, 4097) == 2 * 2 * 2 * 4 and lib.as_colormap_workspace(1, 1 << 30) == 64 * 2 * 4
  assert lib.as_image_to_cv(None, 1, 3, 4, 4, 1, 0.0, 0, nat.ptr(out), st) != 0
  assert lib.as_image_to_cv(nat.ptr(x), 1, 2, 4, 4, 1, 0.0, 0, nat.ptr(out), st) != 0 and b"C 2" in lib.as_last_error()
  assert lib.as_image_to_cv(nat.ptr(x), 1, 1, 4, 0, 1, 0.0, 0, nat.ptr(out), st) != 0
  assert lib.as_image_to_cv(nat.ptr(x), 1, 1, 4, 4, 0, 0.0, 0, nat.c_vp(out.data_ptr() + 1), st) != 0
  torch.cuda.synchronize()
  assert guards_untouched(buf)
  with pytest.raises(RuntimeError, match="must be a tensor on"):
    V.DisparityPainter(4, 4, device=DEV).paint(x.cpu())
  with pytest.raises(RuntimeError, match="expected"):
    V.DisparityPainter(4, 4, device=DEV).paint(torch.zeros(2, 1, 4, 4, device=DEV))


@pytest.mark.parametrize("vmin,vmax", [(0, R.R115), (None, None)], ids=["fixed", "auto"])
def test_painter_in_a_captured_graph_replays_new_contents(vmin, vmax):
  shape = R.SHAPES[2]
  contents = [R.make_case(shape, k) * np.float32(s) for k, s in (("plain", 1.0), ("edges115", 1.0), ("plain", 0.25))]
  painter = V.DisparityPainter(shape[2], shape[3], batch=2, cmap="inferno", vmin=vmin, vmax=vmax, device=DEV)
  eager = [painter.paint(torch.from_numpy(c).to(DEV)).clone() for c in contents]
  static = torch.from_numpy(contents[0]).to(DEV)
  colour_host = np.stack([R.make_image(3, (shape[2], shape[3])), R.make_image(3, (shape[2], shape[3]), seed=1)])
  colour = torch.from_numpy(colour_host).to(DEV)
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    painter.paint(static)                                  # warm-up outside the capture
  torch.cuda.synchronize()
  before = torch.cuda.memory_allocated()
  painter.paint(static)
  painter.rgb(colour)
  assert torch.cuda.memory_allocated() == before, "paint() or rgb() allocated"
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):     # one stream: a linear graph
    image = painter.paint(static)
    left = painter.rgb(colour)
  for c, want, scale in zip(contents, eager, (1.0, 0.5, 0.25)):
    static.copy_(torch.from_numpy(c))
    colour.copy_(torch.from_numpy(colour_host * np.float32(scale)))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(image, want)
    assert same(left.cpu().numpy(), np.stack([R.to_cv_rgb(colour_host[b] * np.float32(scale)) for b in range(2)]))


def test_reference_named_wrappers_from_device_and_cpu_tensors(fixture):
  shape = R.SHAPES[2]
  x = R.make_case(shape, "plain")
  auto = R.case_name(shape, ("plain", None, None, "magma"))
  for put in (lambda a: torch.from_numpy(a).to(DEV), torch.from_numpy):
    got = V.apply_cmap(put(x), cmap="magma")
    assert got.dtype == np.float64 and same(got, fixture["rgba__" + auto])
    for b in range(shape[0]):
      assert same(V.visualize_disp_cv(put(x[b])), fixture["u8__" + auto][b])             # the default map is magma
      tb = V.visualize_disp_tensorboard(put(x[b]))
      assert tb.dtype == np.float32 and same(tb, fixture["f32__" + auto][b])
    fixed = R.case_name(shape, ("plain", 0, R.R115, "inferno"))
    assert same(V.visualize_disp_cv(put(x[1]), cmap="inferno", vmin=0, vmax=0.6 * 192), fixture["u8__" + fixed][1])
    assert same(V.visualize_disp_tensorboard(put(x[0]), vmin=0, vmax=80), fixture["tensorboard_raw__37x53"])
    # apply_cmap's default map is gray; a map of height 3 comes back channel-last from visualize_disp_tensorboard, as there
    small = R.make_case(R.SHAPES[1], "plain")
    assert same(V.apply_cmap(put(small)), fixture["rgba_default__3x7"])
    raw = fixture["tensorboard_raw__3x7"]
    tb = V.visualize_disp_tensorboard(put(small[0]))
    assert raw.shape == (3, 7, 3) and tb.shape == raw.shape and same(tb, raw.astype(np.float32))


@pytest.mark.parametrize("shape", R.SHAPES[:3], ids=lambda s: "b%d_h%d_w%d" % (s[0], s[2], s[3]))
def test_wrappers_at_every_small_shape_and_configuration(fixture, shape):
  """visualize_disp_cv, visualize_disp_tensorboard and apply_cmap through a colour-map OBJECT built from the fixture's table (the
  route a caller with a matplotlib Colormap takes), every configuration, every image of the batch."""
  for config in R.configs_for(shape):
    kind, vmin, vmax, cmap = config
    name = R.case_name(shape, config)
    x = torch.from_numpy(R.make_case(shape, kind))
    cm = R.TableColormap(fixture["table__" + cmap])
    for b in range(shape[0]):
      assert same(V.visualize_disp_cv(x[b], cmap=cm, vmin=vmin, vmax=vmax), fixture["u8__" + name][b]), name
      assert same(V.visualize_disp_cv(x[b].to(DEV), cmap=cmap, vmin=vmin, vmax=vmax), fixture["u8__" + name][b]), name
    if R.stores_float(shape, config):
      assert same(V.apply_cmap(x, vmin=vmin, vmax=vmax, cmap=cm), fixture["rgba__" + name]), name
      for b in range(shape[0]):
        tb = V.visualize_disp_tensorboard(x[b], cmap=cmap, vmin=vmin, vmax=vmax)
        want = fixture["f32__" + name][b]
        assert same(tb, want if shape[2] not in (1, 3) else np.moveaxis(want, 0, -1)), name


class RecordingWriter(object):
  def __init__(self):
    self.images = {}

  def add_image(self, name, image, step):
    self.images[name] = (image, step)


def test_log_images_default_and_colour_mapped(fixture):
  import train
  shape = R.SHAPES[2]
  x = torch.from_numpy(R.make_case(shape, "plain")).to(DEV)
  inputs = {"color_l/0": torch.rand(2, 3, shape[2], shape[3], device=DEV), "gt_disp_l/0": x * 0.5}
  outputs = {"pred_disp_l/0": x, "cost_volume_l/4": torch.rand(2, 12, 3, 4, device=DEV)}
  plain = RecordingWriter()
  train.log_images(plain, inputs, outputs, 7)
  assert sorted(plain.images) == ["color_l/0", "gt_disp_l/0", "pred_disp_l/0"]
  for name, io in (("color_l/0", inputs), ("gt_disp_l/0", inputs), ("pred_disp_l/0", outputs)):
    image, step = plain.images[name]
    assert step == 7 and not image.is_cuda and torch.equal(image, io[name][0].cpu())
  mapped = RecordingWriter()
  train.log_images(mapped, inputs, outputs, 8, disp_cmap="magma")
  assert sorted(mapped.images) == sorted(plain.images)
  assert torch.equal(mapped.images["color_l/0"][0], plain.images["color_l/0"][0])
  image = mapped.images["pred_disp_l/0"][0]
  want = fixture["f32__" + R.case_name(shape, ("plain", None, None, "magma"))][0]
  assert tuple(image.shape) == (3, shape[2], shape[3]) and not image.is_cuda and same(image.numpy(), want)
  assert tuple(mapped.images["gt_disp_l/0"][0].shape) == (3, shape[2], shape[3])
  assert torch.equal(mapped.images["gt_disp_l/0"][0], image), "a scaled map has the same normalised image"


def test_evaluate_model_save_and_video(tmp_path):
  from PIL import Image
  import evaluate_model as E
  from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
  from adaptive_stereo.utils import synthetic as syn
  k, H, W = 4, 64, 128
  fnet, snet = FeatureExtractorNetwork(k), StereoNet(k, 1, 0)
  fnet.load_state_dict(syn.synthetic_state_dict(fnet.state_dict(), seed=123))
  snet.load_state_dict(syn.synthetic_state_dict(snet.state_dict(), seed=123, logit_gain=20.0))
  fnet, snet = fnet.to(DEV), snet.to(DEV)
  left, right = syn.stereo_pair(3, H, W, seed=5)
  gt = torch.from_numpy((np.random.RandomState(5).random_sample((3, 1, H, W)) * 100.0).astype(np.float32))
  gt[:, :, :8] = 0.0                                              # invalid pixels do not count in the EPE
  samples = [{"color_l/0": left[i], "color_r/0": right[i], "gt_disp_l/0": gt[i]} for i in range(3)]
  batches = [{key: torch.stack([s[key] for s in samples[a:b]]) for key in samples[0]} for a, b in ((0, 2), (2, 3))]

  save_folder = str(tmp_path / "weights" / "outputs" / "split")
  assert E.save_outputs(fnet, snet, batches, save_folder, 2) == 3
  folders = sorted(os.listdir(save_folder))
  assert "pred_disp_l_0" in folders and all(f.startswith("pred_disp_l_") for f in folders)
  for f in folders:
    assert sorted(os.listdir(os.path.join(save_folder, f))) == ["0000.pt", "0001.pt", "0002.pt"], f
  preds = [torch.load(E.get_save_filename(save_folder, "pred_disp_l/0", i)) for i in range(3)]
  assert all(tuple(p.shape) == (1, H, W) and not p.is_cuda for p in preds)

  video = str(tmp_path / "video")
  epes = E.write_video_frames(samples, save_folder, video, frames=-1)
  assert sorted(os.listdir(video)) == sorted(["epe.csv"] + ["%s_%05d.png" % (n, i) for n in ("left", "gt", "pred") for i in range(3)])
  painter = V.DisparityPainter(H, W, cmap="inferno", vmin=0, vmax=0.6 * 192, order="rgb", device=DEV)
  for i in range(3):
    for name, want in (("pred", painter.paint(preds[i].to(DEV)).cpu().numpy()[0]), ("gt", painter.paint(gt[i].to(DEV)).cpu().numpy()[0]),
                       ("left", painter.rgb(left[i].to(DEV).contiguous()).cpu().numpy()[0])):
      got = np.asarray(Image.open(os.path.join(video, "%s_%05d.png" % (name, i))))
      assert same(got, want), (name, i)
    valid = gt[i] > 0
    assert abs(epes[i] - float((preds[i] - gt[i]).abs()[valid].mean())) <= 1e-4 * epes[i]
  rows = list(csv.reader(open(os.path.join(video, "epe.csv"))))
  assert len(rows) == 4 and rows[0] == ["frame", "epe"] and [r[0] for r in rows[1:]] == ["0", "1", "2"]
  assert len(E.write_video_frames(samples, save_folder, str(tmp_path / "two"), frames=2)) == 2
  with pytest.raises(RuntimeError, match="display"):
    opt = E.make_parser().parse_args(["--mode", "playback", "--load_weights_folder", str(tmp_path), "--split", "s",
                                      "--dataset_name", "none"])
    E.main(opt)
