"""adaptive_stereo.lidar (csrc/lidar.hip) against tests/lidar_ref.py on EVERY pixel, BIT FOR BIT (depth, disp, disp_u16), and
against the reference's own outputs (tests/golden/lidar_gt.npz) on columns 1..W-2: columns 0 and W-1, 2/131 of the map, are the
only pixels left out, because the reference merges pixel (r, W-1) with pixel (r+1, 0) when it looks for duplicates.

What the cases are for:
  general   75 x 131 (rows end mid-wave), 3001 points (no multiple of 64, more than one workgroup): x < 0, -0.0, NaN, +inf, points
            behind the camera that land in bounds (q2 < 0), several points per pixel, depths one ulp either side of 80 m.
  dyadic    q0/q2 exactly k + 0.5 for even and odd k: fails with round() in place of rint.
  device    a second frame on the same object, a window followed by a full frame, every point on one pixel, a disparity that
            does not fit uint16, a captured graph replayed with new points and counts, a tail beyond counts[b] that is never read,
            the fused metrics, the export script, and the errors raised before any launch.
"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import GOLDEN_DIR, parity_note
from adaptive_stereo import _native as nat
from adaptive_stereo.lidar import KittiCalibration, LidarGroundTruth, LidarFrame, load_velodyne_bin
import lidar_ref as R

DEV = "cuda:0"
F = np.float32
WINDOW = (3, 5, 64, 96)


@functools.lru_cache(maxsize=None)
def _fixture():
  return np.load(os.path.join(GOLDEN_DIR, "lidar_gt.npz"), allow_pickle=False)


@functools.lru_cache(maxsize=None)
def _scan(name, overflow=False):
  s = R.make_scan(name, overflow)
  s.setflags(write=False)
  return s


@functools.lru_cache(maxsize=None)
def _calib(name):
  P = R.projections(name)
  return KittiCalibration(P[2], P[3], R.SCANS[name][:2], R.file_calibration(name)["P_rect_02"][0, 0])


def _want(name, pts, cam, vd, quantize, window=None):
  """(depth, disp, u16, overflow) of the restatement for one image."""
  H, W = R.SCANS[name][:2]
  depth = R.depth_map(R.projections(name)[cam], pts, (H, W), bool(vd))
  if window is not None:
    i0, j0, h, w = window
    depth = depth[i0:i0 + h, j0:j0 + w]
  return R.disparity(depth, R.bf(name), quantize)


@functools.lru_cache(maxsize=None)
def _want_scan(name, cam, vd, quantize):
  return _want(name, _scan(name), cam, vd, quantize)


def _dev(a, dtype=None):
  t = torch.from_numpy(np.array(a, order="C"))                     # a copy: the cached scans are read-only
  return (t if dtype is None else t.to(dtype)).to(DEV)


def _counts(*n):
  return torch.tensor(n, dtype=torch.int32, device=DEV)


def _bits(a):
  return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _same(frame, b, want, what):
  """image b of a LidarFrame against (depth, disp, u16, overflow) of the restatement: every pixel, every bit"""
  assert isinstance(frame, LidarFrame)
  depth, disp, q, over = want
  got = (frame.depth[b, 0].cpu().numpy(), frame.disp[b, 0].cpu().numpy(), frame.disp_u16[b].cpu().numpy())
  assert got[2].dtype == np.uint16
  for g, w, field in zip(got, (depth, disp, q), ("depth", "disp", "disp_u16")):
    assert g.shape == w.shape, "%s %s: shape %s, expected %s" % (what, field, g.shape, w.shape)
    bad = (_bits(g) != _bits(w)) if field != "disp_u16" else (g != w)
    assert not bad.any(), "%s %s: %d of %d pixels differ, first %r" % (what, field, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist())
  assert int(frame.overflow[b]) == over, "%s: overflow %d, expected %d" % (what, int(frame.overflow[b]), over)


# ---- 1. the two fixture scans ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantize", [True, False])
@pytest.mark.parametrize("vd", [1, 0])
@pytest.mark.parametrize("cam", [2, 3])
@pytest.mark.parametrize("name", sorted(R.SCANS))
def test_device_equals_the_restatement_on_every_pixel(name, cam, vd, quantize):
  H, W, N, _ = R.SCANS[name]
  gt = LidarGroundTruth(_calib(name), batch=1, max_points=N, device=DEV)
  frame = gt.project(_dev(_scan(name)[None]), _counts(N), cam=cam, vel_depth=bool(vd), quantize=quantize)
  assert tuple(frame.disp.shape) == (1, 1, H, W) and tuple(frame.depth.shape) == (1, 1, H, W) and tuple(frame.disp_u16.shape) == (1, H, W)
  assert frame.metrics is None
  want = _want_scan(name, cam, vd, quantize)
  assert (want[1] > 0).sum() > 200 and want[3] == 0
  _same(frame, 0, want, "%s cam %d vel_depth %d quantize %d" % (name, cam, vd, quantize))
  assert frame.disp.data_ptr() == gt._disp.data_ptr() and frame.depth.data_ptr() == gt._depth.data_ptr()      # views alias the buffers


@pytest.mark.parametrize("vd", [1, 0])
@pytest.mark.parametrize("cam", [2, 3])
@pytest.mark.parametrize("name", sorted(R.SCANS))
def test_device_equals_the_reference_off_the_edge_columns(name, cam, vd):
  H, W, N, _ = R.SCANS[name]
  z = _fixture()
  gt = LidarGroundTruth(_calib(name), batch=1, max_points=N, device=DEV)
  frame = gt.project(_dev(_scan(name)[None]), _counts(N), cam=cam, vel_depth=bool(vd))
  with np.errstate(over="ignore"):
    want = z["depth__%s__cam%d__vd%d" % (name, cam, vd)].astype(F)
  diff = _bits(frame.depth[0, 0].cpu().numpy()) != _bits(want)
  assert not diff[:, 1:W - 1].any(), "%d interior pixels differ from the reference" % int(diff[:, 1:W - 1].sum())
  note = dict(edge_column_pixels_differing=int(diff.sum()), of=2 * H)
  if vd:
    q = z["export__%s__cam%d" % (name, cam)]
    qd = frame.disp_u16[0].cpu().numpy() != q
    assert not qd[:, 1:W - 1].any(), "%d interior pixels of the export differ from the reference" % int(qd[:, 1:W - 1].sum())
    dec = (q.astype(F) * F(1.0 / 128))[:, 1:W - 1]                                 # what the dataset layer reads from the file
    assert np.array_equal(_bits(frame.disp[0, 0].cpu().numpy()[:, 1:W - 1]), _bits(dec))
    note["export_edge_column_pixels_differing"] = int(qd.sum())
  parity_note("lidar_device_vs_reference_%s_cam%d_vd%d" % (name, cam, vd), **note)


# ---- 2. device-only cases -------------------------------------------------------------------------------------------------
def test_second_frame_does_not_see_the_first():
  name, (H, W, N, _) = "general", R.SCANS["general"]
  gt = LidarGroundTruth(_calib(name), batch=2, max_points=N, device=DEV)
  points = _dev(np.stack([_scan(name), _scan(name)[::-1]]))
  empty = _want(name, _scan(name)[:0], 2, 1, True)
  frame = gt.project(points, _counts(N, 0))
  _same(frame, 0, _want_scan(name, 2, 1, True), "frame 1 image 0")
  _same(frame, 1, empty, "frame 1 image 1 (counts = 0)")
  assert not frame.disp[1].any()
  frame = gt.project(points, _counts(64, N))
  _same(frame, 0, _want(name, _scan(name)[:64], 2, 1, True), "frame 2 image 0 (64 points)")
  _same(frame, 1, _want_scan(name, 2, 1, True), "frame 2 image 1 (the scan in reverse order: the minimum ignores order)")
  one = gt.project(points[:1], _counts(0))                                        # a smaller batch on the same buffers
  assert tuple(one.disp.shape) == (1, 1, H, W) and not one.depth.any()


def test_window_then_full_frame():
  name, (H, W, N, _) = "general", R.SCANS["general"]
  i0, j0, h, w = WINDOW
  gt = LidarGroundTruth(_calib(name), batch=1, max_points=N, device=DEV)
  points = _dev(_scan(name)[None])
  for vd, quantize in ((1, True), (0, False)):
    frame = gt.project(points, _counts(N), cam=3, window=WINDOW, vel_depth=bool(vd), quantize=quantize)
    assert tuple(frame.disp.shape) == (1, 1, h, w) and frame.disp.is_contiguous() and tuple(frame.disp_u16.shape) == (1, h, w)
    _same(frame, 0, _want(name, _scan(name), 3, vd, quantize, WINDOW), "window vel_depth %d" % vd)
    full = gt.project(points, _counts(0), cam=3)                                  # nothing projected: a key the window pass had left
    assert not full.depth.any() and not full.disp_u16.cpu().numpy().any()                       # behind outside the window would show here
  _same(gt.project(points, _counts(N), cam=3), 0, _want_scan(name, 3, 1, True), "full frame after the windows")


def test_every_point_on_one_pixel():
  name, n = "dyadic", 4096
  r = np.random.RandomState(5)
  pts = np.stack([0.45 + 0.1 * r.rand(n), np.full(n, 0.25), np.full(n, 4.0), r.rand(n)], axis=1).astype(F)      # 19.6 < q0/q2 < 20.4
  gt = LidarGroundTruth(_calib(name), batch=1, max_points=n, device=DEV)
  for vd in (1, 0):
    frame = gt.project(_dev(pts[None]), _counts(n), vel_depth=bool(vd))
    want = _want(name, pts, 2, vd, True)
    assert (want[0] != 0).sum() == 1 and (not vd or want[0].max() == pts[:, 0].min())
    _same(frame, 0, want, "contention vel_depth %d" % vd)


@pytest.mark.parametrize("name", sorted(R.SCANS))
def test_disparity_beyond_uint16_is_zero_and_counted(name):
  H, W, N, _ = R.SCANS[name]
  pts = _scan(name, True)
  gt = LidarGroundTruth(_calib(name), batch=1, max_points=N, device=DEV)
  for quantize in (True, False):
    frame = gt.project(_dev(pts[None]), _counts(N), quantize=quantize)
    want = _want(name, pts, 2, 1, quantize)
    raw = R.depth_map(R.projections(name)[2], pts, (H, W), True)
    at = np.argwhere(raw == pts[N - 1, 0])
    assert want[3] == 1 and len(at) == 1                                          # the planted point is alone the nearest of its pixel
    _same(frame, 0, want, "%s overflow quantize %d" % (name, quantize))
    v, u = at[0]
    assert int(frame.overflow[0]) == 1
    assert float(frame.depth[0, 0, v, u]) == 0 and float(frame.disp[0, 0, v, u]) == 0 and int(frame.disp_u16[0].cpu().numpy()[v, u]) == 0


def test_captured_graph_replays_with_new_points_and_counts():
  name, (H, W, N, _) = "general", R.SCANS["general"]
  cap = 3200
  gt = LidarGroundTruth(_calib(name), batch=1, max_points=cap, device=DEV)
  host = np.full((1, cap, 4), np.nan, dtype=F)
  host[0, :N] = _scan(name)
  static_points, static_counts = _dev(host), _counts(N)
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    gt.project(static_points, static_counts)                  # warm-up outside the capture
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):     # one stream: a linear graph
    frame = gt.project(static_points, static_counts)          # allocates nothing, synchronises nothing: capturable
  graph.replay()
  torch.cuda.synchronize()
  _same(frame, 0, _want_scan(name, 2, 1, True), "replay 1")
  second = _scan(name, True)[::-1][:1777]
  host[0, :1777] = second                                     # rows 1777..3000 keep the first scan: beyond counts, never read
  static_points.copy_(torch.from_numpy(host))
  static_counts.copy_(torch.tensor([1777], dtype=torch.int32))
  graph.replay()
  torch.cuda.synchronize()
  _same(frame, 0, _want(name, second, 2, 1, True), "replay 2 (new points, new counts)")


def test_tail_beyond_counts_is_never_read():
  name, (H, W, N, _) = "general", R.SCANS["general"]
  cap = 4096
  host = np.full((1, cap, 4), np.nan, dtype=F)
  host[0, :N] = _scan(name)
  P = R.projections(name)[2]
  near = [R.point_at(P, 0.3, u, v) + [0.0] for v in range(2, H, 9) for u in range(2, W, 9)]       # would win their pixels if read
  host[0, N + 100:N + 100 + len(near)] = np.array(near, dtype=F)
  gt = LidarGroundTruth(_calib(name), batch=1, max_points=cap, device=DEV)
  _same(gt.project(_dev(host), _counts(N)), 0, _want_scan(name, 2, 1, True), "NaN and near points beyond counts")
  _same(gt.project(_dev(host), _counts(cap)), 0, _want(name, host[0], 2, 1, True), "the same tail inside counts")
  _same(gt.project(_dev(host), _counts(cap + 5)), 0, _want(name, host[0], 2, 1, True), "counts beyond Nmax reads Nmax points")


# ---- 3. metrics -----------------------------------------------------------------------------------------------------------
def _planted_pred(gt_disp, seed):
  """gt + seeded noise, then |err| = 2, 3, 4, 5 exactly and one ulp either side at twelve pixels with 0 < gt < 1.9, where
  pred = gt - t is exact in fp32 (checked here, on the host arithmetic alone)"""
  r = np.random.RandomState(seed)
  pred = (gt_disp + 2.5 * r.standard_normal(gt_disp.shape)).astype(F)
  flat, g = pred.reshape(-1), gt_disp.reshape(-1)
  where = np.nonzero((g > 0) & (g < F(1.9)))[0]
  targets = [t for k in (2, 3, 4, 5) for t in (np.nextafter(F(k), F(0)), F(k), np.nextafter(F(k), F(9)))]
  assert len(where) >= len(targets)
  for i, t in zip(where[:len(targets)], targets):
    p = np.float64(g[i]) - np.float64(t)
    assert np.float64(F(p)) == p and np.abs(F(F(p) - g[i])) == t
    flat[i] = F(p)
  return pred


def test_metrics_counts_exact_sum_bounded_and_repeatable():
  name, (H, W, N, _) = "general", R.SCANS["general"]
  i0, j0, h, w = WINDOW
  gt = LidarGroundTruth(_calib(name), batch=2, max_points=N, device=DEV)
  scans = [_scan(name), _scan(name, True)[:2000]]
  points = _dev(np.stack([scans[0], _scan(name, True)]))
  counts = _counts(N, 2000)
  want = [_want(name, s, 2, 1, True, WINDOW) for s in scans]
  gt_disp = np.stack([x[1] for x in want])[:, None]
  pred = _planted_pred(gt_disp, seed=11)
  pred_dev = _dev(pred)
  frame = gt.project(points, counts, window=WINDOW, pred_disp=pred_dev)
  assert tuple(frame.metrics.shape) == (2, 6) and frame.metrics.dtype == torch.float32
  first = frame.metrics.cpu().numpy().copy()
  for b in range(2):
    _same(frame, b, want[b], "metrics image %d" % b)
    s, c = R.metrics(pred[b, 0], gt_disp[b, 0])
    n = c[0]
    assert 100 < n < 3000 and c[1] > c[2] > c[3] > c[4] > 0
    print("image %d: counts %r device %r, sum %.9g device %.9g" % (b, c, first[b, 1:].tolist(), s, first[b, 0]))
    assert first[b, 1:].tolist() == [float(v) for v in c], "image %d: counts %r, expected %r" % (b, first[b, 1:].tolist(), c)
    assert abs(float(first[b, 0]) - s) <= n * 2.0 ** -24 * s, "image %d: error sum %.9g, fp64 %.9g" % (b, first[b, 0], s)
  again = gt.project(points, counts, window=WINDOW, pred_disp=pred_dev).metrics.cpu().numpy()
  assert np.array_equal(first.view(np.uint32), again.view(np.uint32))              # fixed summation order: the same bits

  frame = gt.project(points, counts, window=WINDOW, pred_disp=pred_dev)
  k = frame.disp.numel()
  out6 = torch.zeros(6, dtype=torch.float32, device=DEV)
  ws = torch.empty(nat.load().as_eval_metrics_workspace(k), dtype=torch.float32, device=DEV)
  nat.call("as_eval_metrics", nat.ptr(pred_dev), nat.ptr(frame.disp), k, nat.ptr(out6), nat.ptr(ws), nat.stream())
  out6 = out6.cpu().numpy()
  assert out6[1:].tolist() == first[:, 1:].sum(axis=0).tolist()                    # the batch-level kernel on the same tensors
  total = float(first[:, 0].astype(np.float64).sum())
  assert abs(float(out6[0]) - total) <= out6[1] * 2.0 ** -24 * total


# ---- 4. the export script -------------------------------------------------------------------------------------------------
def test_export_script_on_a_two_frame_tree(tmp_path, monkeypatch):
  import export_gt_disp as script
  name, (H, W, N, _) = "general", R.SCANS["general"]
  z = _fixture()
  root = tmp_path / "kitti_data_raw"
  date = root / R.DATES[name]
  drive = date / R.DRIVES[name]
  R.write_calibration(str(date), name)
  for sub in ("image_02", "image_03", "velodyne_points"):
    os.makedirs(str(drive / sub / "data"))
  for sub in ("image_02", "image_03"):
    for frame in (R.FRAME, "0000000006"):
      (drive / sub / "data" / (frame + ".jpg")).write_bytes(b"")                   # never decoded
  velo = drive / "velodyne_points" / "data" / (R.FRAME + ".bin")
  _scan(name).tofile(str(velo))
  pinned = load_velodyne_bin(str(velo))
  assert tuple(pinned.shape) == (N, 4) and pinned.is_pinned() and np.array_equal(_bits(pinned.numpy()), _bits(_scan(name)))
  os.makedirs(str(drive / "disp_02"))
  np.save(str(drive / "disp_02" / "stale.npy"), np.zeros(3))
  monkeypatch.chdir(tmp_path)
  written, skipped = script.export_gt_disp(str(root), cleanup_old=True, batch=2, device=DEV)
  assert (written, skipped) == (1, 1)
  assert not (drive / "disp_02" / "stale.npy").exists()
  missing = (tmp_path / "no_groundtruth.txt").read_text().splitlines()
  assert len(missing) == 1 and missing[0].endswith(os.path.join("image_02", "data", "0000000006.jpg"))
  for cam in (2, 3):
    assert not (drive / ("disp_0%d" % cam) / "data" / "0000000006.npy").exists()
    q = np.load(str(drive / ("disp_0%d" % cam) / "data" / (R.FRAME + ".npy")))
    assert q.dtype == np.uint16 and q.shape == (H, W)
    assert np.array_equal(q, _want_scan(name, cam, 1, True)[2])                    # the restatement everywhere
    assert np.array_equal(q[:, 1:W - 1], z["export__%s__cam%d" % (name, cam)][:, 1:W - 1])      # the reference's own file off the edges


# ---- 5. errors raised in Python, before any launch ------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch():
  name, (H, W, N, _) = "general", R.SCANS["general"]
  gt = LidarGroundTruth(_calib(name), batch=1, max_points=N, device=DEV)
  points, counts = _dev(_scan(name)[None]), _counts(N)
  bad = [
    dict(points=points.double()),                                                  # wrong dtype
    dict(counts=counts.long()),
    dict(points=points.cpu()),                                                     # CPU tensor
    dict(counts=counts.cpu()),
    dict(counts=_counts(N, N)),                                                    # counts longer than the batch
    dict(points=_dev(np.zeros((2, 8, 4), F)), counts=_counts(8, 8)),               # batch beyond the buffers
    dict(points=_dev(np.zeros((1, N + 1, 4), F))),                                 # Nmax > max_points
    dict(points=points[:, :, :3]),                                                 # not [B,N,4] (and not contiguous)
    dict(window=(0, 0, H + 1, W)), dict(window=(-1, 0, 8, 8)), dict(window=(70, 100, 8, 32)), dict(window=(0, 0, 0, 8)),
    dict(pred_disp=torch.zeros(1, 1, H, W + 1, device=DEV)),
    dict(pred_disp=torch.zeros(1, 1, H, W)),
  ]
  for kw in bad:
    args = dict(points=points, counts=counts)
    args.update(kw)
    with pytest.raises(RuntimeError):
      gt.project(**args)
  with pytest.raises(ValueError):
    gt.project(points, counts, cam=1)
  with pytest.raises(RuntimeError):
    LidarGroundTruth(_calib(name), device="cpu")
  _same(gt.project(points, counts), 0, _want_scan(name, 2, 1, True), "after the refused calls")      # nothing was launched
