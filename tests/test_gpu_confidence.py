"""csrc/confidence.hip (as_disp_confidence, as_sparsification), the confidence gate of csrc/pointcloud.hip
(as_disp_to_points_gated) and adaptive_stereo/confidence.py + the gated DepthProjector on the GPU, against tests/confidence_ref.py
(held to torch's float64 soft-max and bracketed by tests/test_confidence_ref_cpu.py).

  maps     inside the derived bounds of confidence_ref.stage (worst |err| / bound <= 1, printed), the quiet NaN exactly at the bad
           columns and nowhere else, every output written between sentinel guard floats
  gate     GIVEN confidence maps, so every decision is exact: depth, xyz, records, voxel, count, n, dropped and rejected bit for
           bit against pointcloud_ref with `valid &= conf >= conf_min`
  bins     count, bad and skipped exact; abs_err within n 2^-53 of its bin's sum (math.fsum)
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import confidence_ref as cr
import pointcloud_ref as pr
from adaptive_stereo import _native as nat
from adaptive_stereo import confidence as conf_mod
from adaptive_stereo.pointcloud import DepthProjector, StereoCamera, VoxelCloud

DEV = "cuda:0"
F = np.float32
SENTINEL = -7777.0
GUARD = 64
CASES = [(shape, gain) for shape in cr.SHAPES for gain in cr.GAINS]
IDS = [cr.case_name(s, g) for s, g in CASES]


def bits(t):
  return t.contiguous().view(torch.int32)


def _np_bits(a):
  return np.ascontiguousarray(a, dtype=F).view(np.int32)


class Guarded(object):
  """`count` buffers of n elements each inside one sentinel-filled allocation, GUARD elements between and around them"""

  def __init__(self, count, n, dtype=torch.float32):
    self.n, self.count = n, count
    self.raw = torch.full((count * (n + GUARD) + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    self.views = [self.raw[GUARD + i * (n + GUARD):GUARD + i * (n + GUARD) + n] for i in range(count)]

  def guards_intact(self):
    mask = torch.ones_like(self.raw, dtype=torch.bool)
    for i in range(self.count):
      mask[GUARD + i * (self.n + GUARD):GUARD + i * (self.n + GUARD) + self.n] = False
    return bool((self.raw[mask] == SENTINEL).all())


# ================================================================================================= as_disp_confidence
def run_maps(x, which=cr.MAP_NAMES):
  """as_disp_confidence on a device volume -> {name: [B,H,W] device tensor} for the requested outputs, each between guards"""
  B, D, H, W = x.shape
  g = Guarded(3, B * H * W)
  views = dict(zip(cr.MAP_NAMES, g.views))
  nat.call("as_disp_confidence", nat.ptr(x), B, D, H, W, *([nat.ptr(views[k]) if k in which else None for k in cr.MAP_NAMES] +
                                                          [nat.stream()]))
  torch.cuda.synchronize()
  assert g.guards_intact(), "a write outside the outputs"
  for k in cr.MAP_NAMES:
    if k not in which:
      assert bool((views[k] == SENTINEL).all()), "%s was not requested and was written" % k
  return {k: views[k].reshape(B, H, W) for k in which}


def check_maps(got, s, what):
  worst = {}
  for k, t in got.items():
    worst[k] = cr.worst_ratio(t.cpu().numpy(), s[k], s["e_" + k], s["bad"])
  print("%s: worst |err| / bound %s" % (what, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
  assert all(v <= 1.0 for v in worst.values()), (what, worst)


@pytest.fixture(scope="module")
def stages():
  """the fp64 reference of every case, computed once"""
  out = {}
  for shape, gain in CASES:
    vol = cr.make_volume(shape, gain)
    out[(shape, gain)] = (vol, cr.stage(vol))
  return out


@pytest.mark.parametrize("shape,gain", CASES, ids=IDS)
def test_maps_inside_their_bounds(stages, shape, gain):
  vol, s = stages[(shape, gain)]
  x = torch.from_numpy(vol).to(DEV)
  together = run_maps(x)
  check_maps(together, s, cr.case_name(shape, gain))
  for k in cr.MAP_NAMES:                                   # each output alone: the same bits, nothing else written
    alone = run_maps(x, (k,))
    assert torch.equal(bits(alone[k]), bits(together[k])), k
  # the first maximum behind mass is as_softargmax_fwd's argmax wherever the column is finite
  B, D, H, W = shape
  pred = torch.empty(B, H, W, device=DEV)
  am = torch.empty(B, H, W, dtype=torch.int32, device=DEV)
  nat.call("as_softargmax_fwd", nat.ptr(x), B, D, H, W, nat.ptr(pred), nat.ptr(am), None, nat.stream())
  finite = np.isfinite(vol).all(axis=1)
  assert np.array_equal(am.cpu().numpy()[finite], s["a"][finite])


def test_nan_stays_in_its_pixel():
  shape = (2, 12, 5, 67)
  clean = cr.make_volume(shape, 1.0)
  bad = cr.bad_columns(clean)
  clean[:, :, bad[0] | bad[1]] = 0.5                       # the same pixels cleaned in both images
  dirty = clean.copy()
  spots = [(0, 0, 0), (0, 2, 33), (1, 4, 66), (1, 0, 64)]
  for i, (b, y, x) in enumerate(spots):
    dirty[b, (5 * i) % 12, y, x] = [np.nan, np.inf, np.nan, np.inf][i]
  a, b = run_maps(torch.from_numpy(clean).to(DEV)), run_maps(torch.from_numpy(dirty).to(DEV))
  hit = np.zeros((2, 5, 67), bool)
  for s in spots:
    hit[s] = True
  for k in cr.MAP_NAMES:
    ga, gb = a[k].cpu().numpy(), b[k].cpu().numpy()
    assert not np.isnan(ga).any()
    assert (_np_bits(gb)[hit] == cr.QNAN_BITS).all()
    assert np.array_equal(_np_bits(ga)[~hit], _np_bits(gb)[~hit]), "%s: a neighbour of a bad column changed" % k


def test_confidence_errors_return_before_any_launch():
  lib = nat.load()
  x = torch.zeros(1, 3, 4, 4, device=DEV)
  g = Guarded(3, 16)
  p = [nat.ptr(v) for v in g.views]
  for args in ((None, 1, 3, 4, 4, p[0], p[1], p[2]), (nat.ptr(x), 0, 3, 4, 4, p[0], p[1], p[2]), (nat.ptr(x), 1, 0, 4, 4, p[0], p[1], p[2]),
               (nat.ptr(x), 1, 65, 4, 4, p[0], p[1], p[2]), (nat.ptr(x), 65536, 3, 4, 4, p[0], p[1], p[2]),
               (nat.ptr(x), 1, 3, 4, 0, p[0], p[1], p[2]), (nat.ptr(x), 1, 3, 4, 4, None, None, None)):
    assert lib.as_disp_confidence(*(args + (nat.stream(),))) == -1
  torch.cuda.synchronize()
  assert bool((g.raw == SENTINEL).all())
  with pytest.raises(RuntimeError, match="contiguous"):
    conf_mod.disparity_confidence(torch.zeros(1, 3, 4, 6, device=DEV).transpose(2, 3))
  with pytest.raises(RuntimeError):
    conf_mod.disparity_confidence(torch.zeros(1, 3, 4, 4, device=DEV, dtype=torch.float64))
  with pytest.raises(RuntimeError, match="no CPU path"):
    conf_mod.disparity_confidence(torch.zeros(1, 3, 4, 4))


def test_confidence_in_a_captured_graph_follows_new_contents(stages):
  shape = (2, 12, 5, 67)
  first, s1 = stages[(shape, 1.0)]
  second, s2 = stages[(shape, 50.0)]
  static = torch.from_numpy(first).to(DEV)
  g = Guarded(3, 2 * 5 * 67)
  side = torch.cuda.Stream()

  def launch():
    nat.call("as_disp_confidence", nat.ptr(static), 2, 12, 5, 67, nat.ptr(g.views[0]), nat.ptr(g.views[1]), nat.ptr(g.views[2]),
             nat.stream())
  with torch.cuda.stream(side):
    launch()                                               # warm-up outside the capture
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):     # one stream: a linear graph
    launch()
  for vol, s in ((first, s1), (second, s2)):
    static.copy_(torch.from_numpy(vol))
    g.views[0].fill_(SENTINEL); g.views[1].fill_(SENTINEL); g.views[2].fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    check_maps({k: v.reshape(2, 5, 67) for k, v in zip(cr.MAP_NAMES, g.views)}, s, "replay")
    assert g.guards_intact()


def test_module_function_serves_every_kind(stages):
  shape = (4, 12, 24, 78)
  vol, s = stages[(shape, 1.0)]
  x = torch.from_numpy(vol).to(DEV)
  out = conf_mod.disparity_confidence(x, kinds=("entropy", "fcs", "pmax", "mass"))
  assert sorted(out) == ["entropy", "fcs", "mass", "pmax"] and all(tuple(t.shape) == (4, 24, 78) for t in out.values())
  check_maps(dict(pmax=out["pmax"], cent=out["entropy"], mass=out["mass"]), s, "disparity_confidence")
  fm = torch.empty(4, 24, 78, device=DEV)
  nat.call("as_fcs_scores", nat.ptr(x), 4, 12, 24, 78, nat.ptr(fm), None, None, 0, None, None, nat.stream())
  assert torch.equal(bits(out["fcs"]), bits(fm))
  only = conf_mod.disparity_confidence(x, kinds=("mass",))
  assert list(only) == ["mass"] and torch.equal(bits(only["mass"]), bits(out["mass"]))
  up = conf_mod.upsample_confidence(only["mass"][:, :, :77].contiguous()[:1], 96, 300)
  want = torch.empty(1, 1, 96, 300, device=DEV)
  nat.call("as_upsample_bilinear_fwd", nat.ptr(only["mass"][:, :, :77].contiguous()), 1, 24, 77, nat.ptr(want), 96, 300, 1.0, nat.stream())
  assert torch.equal(bits(up), bits(want)) and conf_mod.upsample_confidence(only["mass"][:1].contiguous(), 96, 300, out=want) is want


# ================================================================================================= the gate
def _camera(H, W, fx=721.5, baseline=0.54):
  return StereoCamera(fx, fx * 1.03, 0.37 * W + 0.3, 0.45 * H + 0.7, baseline)      # centre non-integer and off-centre


def _consts(cam, s):
  return pr.camera_constants(cam.fx, cam.fy, cam.cx, cam.cy, cam.baseline, s)


def _scene(B, H, W, s, seed):
  """depth log-uniform from 2 m to 195 m (a fifth beyond depth_trunc), constant over each output pixel's block; some disparities
  0, negative and NaN"""
  rs = np.random.RandomState(seed)
  n = 1 << s
  coarse = np.exp(rs.uniform(np.log(2.0), np.log(190.0), (B, 1, H // n + 1, W // n + 1)))
  coarse[rs.rand(*coarse.shape) < 0.03] = 0.0
  coarse[rs.rand(*coarse.shape) < 0.02] = -3.0
  coarse[rs.rand(*coarse.shape) < 0.02] = np.nan
  return np.kron(coarse, np.ones((n, n)))[:, :, :H, :W].astype(F)


CONF_MIN = F(0.4)


def _given_conf(B, h, w, valid, seed, conf_min=CONF_MIN):
  """uniform confidences with the decision edges planted on pixels that are valid by depth, in EVERY image: conf == conf_min
  (kept), its fp32 neighbour below (rejected), NaN (rejected), +inf (kept), -inf (rejected)"""
  rs = np.random.RandomState(seed)
  conf = rs.rand(B, h, w).astype(F)
  edges = [F(conf_min), np.nextafter(F(conf_min), F(-np.inf), dtype=F), F(np.nan), F(np.inf), F(-np.inf)]
  expect = []
  for b in range(B):
    at = np.flatnonzero(valid[b].reshape(-1))
    at = at[rs.permutation(at.size)[:len(edges) * 2]]
    for i, pix in enumerate(at):
      conf[b].reshape(-1)[pix] = edges[i % len(edges)]
      expect.append((b, pix, i % len(edges) in (0, 3)))
  return conf, expect


def run_gated(proj, disp, rgb, conf, conf_min, b=None, table=True):
  """as_disp_to_points_gated (depth, xyz and the table in ONE launch) + finalize through the projector's buffers"""
  b = disp.shape[0] if b is None else b
  with torch.cuda.device(proj.device):
    nat.call("as_disp_to_points_gated", nat.ptr(disp), nat.ptr(rgb), nat.ptr(conf), float(conf_min), b, proj.H, proj.W, proj.s,
             ctypes.byref(proj._cam), nat.ptr(proj._depth), nat.ptr(proj._xyz), proj.voxel_size, nat.ptr(proj._table) if table else None,
             proj.slots, nat.ptr(proj._rejected), nat.stream())
    if table:
      nat.call("as_voxel_cloud_finalize", nat.ptr(proj._table), b, proj.slots, proj.cap, nat.ptr(proj._records), nat.ptr(proj._voxel),
               nat.ptr(proj._count), nat.ptr(proj._n), nat.ptr(proj._dropped), nat.stream())
  return VoxelCloud(b, proj._records, proj._voxel, proj._count, proj._n, proj._dropped, proj._rejected)


def check_gated(proj, cloud, disp, rgb, conf, conf_min, cam, s, voxel_size=0.15, **depth_args):
  """depth, xyz, rejected and every image's cloud against the reference, bit for bit; returns (reference clouds, gated points)"""
  B = disp.shape[0]
  p = pr.points(disp, _consts(cam, s), s, **depth_args)
  q, rejected = cr.gate(p, conf, conf_min)
  depth = proj._depth[:B, 0].cpu().numpy()
  assert np.array_equal(np.isnan(depth), np.isnan(p["depth"]))
  assert np.array_equal(_np_bits(depth)[~np.isnan(depth)], _np_bits(p["depth"])[~np.isnan(depth)]), "depth"
  want = pr.organized(q)
  xyz = proj._xyz[:B].cpu().numpy()
  assert np.array_equal(_np_bits(xyz), _np_bits(want)), "organised cloud: %d words differ" % int(np.sum(_np_bits(xyz) != _np_bits(want)))
  assert cloud.rejected.tolist() == rejected.tolist(), "rejected %s, reference %s" % (cloud.rejected.tolist(), rejected.tolist())
  colour = None if rgb is None else pr.colour_bytes(rgb, s)
  got = cloud.trim()
  refs = []
  for b in range(B):
    ref = pr.voxel_cloud(q, b, voxel_size, colour)
    g = got[b]
    assert int(cloud.n[b]) == ref["n"] == g["voxel"].shape[0], "image %d: %d voxels, reference %d" % (b, int(cloud.n[b]), ref["n"])
    assert g["dropped"] == ref["dropped"], "image %d: dropped %d, reference %d" % (b, g["dropped"], ref["dropped"])
    vox, cnt, rec = pr.sort_cloud(g["voxel"].cpu().numpy(), g["count"].cpu().numpy(), g["records"].cpu().numpy())
    assert np.array_equal(vox, ref["voxel"]), "image %d: voxel sets differ" % b
    assert np.array_equal(cnt, ref["count"]), "image %d: counts differ" % b
    assert np.array_equal(rec[:, :3], _np_bits(ref["xyz"])), "image %d: mean words differ" % b
    assert np.array_equal(rec[:, 3].view(np.uint32), ref["rgb"]), "image %d: packed colours differ" % b
    refs.append(ref)
  return refs, p, q, rejected


GATE_SHAPES = [(2, 10, 13, 2), (1, 37, 131, 1), (2, 75, 259, 0), (2, 23, 524, 2)]


@pytest.mark.parametrize("depth_scale", [100.0, 0.0])
@pytest.mark.parametrize("colour", [True, False])
@pytest.mark.parametrize("B,H,W,s", GATE_SHAPES)
def test_gated_cloud_bit_exact(B, H, W, s, colour, depth_scale):
  cam = _camera(H, W)
  h, w = H >> s, W >> s
  disp = _scene(B, H, W, s, seed=H + W + s)
  rgb = np.random.RandomState(5).rand(B, 3, H, W).astype(F) if colour else None
  valid = pr.points(disp, _consts(cam, s), s, depth_scale=depth_scale)["valid"]
  conf, expect = _given_conf(B, h, w, valid, seed=H * W)
  proj = DepthProjector(H, W, cam, batch=B, pyramid_scale=s, depth_scale=depth_scale, device=DEV)
  d_disp, d_rgb, d_conf = (None if a is None else torch.from_numpy(a).to(DEV) for a in (disp, rgb, conf))
  cloud = run_gated(proj, d_disp, d_rgb, d_conf, CONF_MIN)
  refs, p, q, rejected = check_gated(proj, cloud, disp, rgb, conf, CONF_MIN, cam, s, depth_scale=depth_scale)
  for b, pix, kept in expect:                              # the planted edges decide what they should
    assert p["valid"][b].reshape(-1)[pix] and q["valid"][b].reshape(-1)[pix] == kept
  assert all(r > 0 for r in rejected) and all(q["valid"][b].sum() > 0 for b in range(B))
  assert (~p["valid"]).sum() > 0                            # some pixels are invalid by depth, whatever their confidence
  if not colour:
    assert int(cloud.records[..., 3].abs().max()) == 0


@pytest.mark.parametrize("colour", [True, False])
def test_gate_wide_open_is_as_disp_to_points_bit_for_bit(colour):
  B, H, W, s = 2, 23, 524, 2
  cam = _camera(H, W)
  disp = _scene(B, H, W, s, seed=11)
  rgb = np.random.RandomState(6).rand(B, 3, H, W).astype(F) if colour else None
  conf = (np.random.RandomState(7).rand(B, H >> s, W >> s).astype(F) - F(0.5)) * F(1e30)
  d_disp, d_rgb, d_conf = (None if a is None else torch.from_numpy(a).to(DEV) for a in (disp, rgb, conf))
  plain, gated = (DepthProjector(H, W, cam, batch=B, pyramid_scale=s, device=DEV) for _ in range(2))
  with torch.cuda.device(plain.device):
    nat.call("as_disp_to_points", nat.ptr(d_disp), nat.ptr(d_rgb), B, H, W, s, ctypes.byref(plain._cam), nat.ptr(plain._depth),
             nat.ptr(plain._xyz), plain.voxel_size, nat.ptr(plain._table), plain.slots, nat.stream())
    nat.call("as_voxel_cloud_finalize", nat.ptr(plain._table), B, plain.slots, plain.cap, nat.ptr(plain._records), nat.ptr(plain._voxel),
             nat.ptr(plain._count), nat.ptr(plain._n), nat.ptr(plain._dropped), nat.stream())
  gated._rejected.fill_(-5)
  cloud = run_gated(gated, d_disp, d_rgb, d_conf, -math.inf)
  torch.cuda.synchronize()
  assert cloud.rejected.tolist() == [0, 0]
  assert torch.equal(bits(gated._depth), bits(plain._depth)) and torch.equal(bits(gated._xyz), bits(plain._xyz))
  assert torch.equal(gated._n, plain._n) and torch.equal(gated._dropped, plain._dropped) and int(plain._n.min()) > 20
  for b in range(B):
    k = int(plain._n[b])
    a = pr.sort_cloud(plain._voxel[b, :k].cpu().numpy(), plain._count[b, :k].cpu().numpy(), plain._records[b, :k].cpu().numpy())
    g = pr.sort_cloud(gated._voxel[b, :k].cpu().numpy(), gated._count[b, :k].cpu().numpy(), gated._records[b, :k].cpu().numpy())
    assert all(np.array_equal(x, y) for x, y in zip(a, g)), "image %d" % b


def test_a_rejected_out_of_range_point_is_not_dropped():
  B, H, W, s = 2, 23, 524, 2
  cam = StereoCamera(0.005, 721.5, 0.37 * W + 0.3, 0.45 * H + 0.7, 0.54 * 721.5 / 0.005)   # fxs = 0.00125: x up to ~5e6 m
  disp = (4.0 + 186.0 * np.random.RandomState(9).rand(B, 1, H, W)).astype(F)
  conf = np.random.RandomState(10).rand(B, H >> s, W >> s).astype(F)
  proj = DepthProjector(H, W, cam, batch=B, pyramid_scale=s, device=DEV)
  cloud = run_gated(proj, torch.from_numpy(disp).to(DEV), None, torch.from_numpy(conf).to(DEV), 0.5)
  refs, p, q, rejected = check_gated(proj, cloud, disp, None, conf, 0.5, cam, s)
  for b in range(B):
    ungated = pr.voxel_cloud(p, b, 0.15)
    assert refs[b]["dropped"] >= 20 and ungated["dropped"] >= refs[b]["dropped"] + 20     # rejected ones among the out-of-range
    assert cloud.dropped.tolist()[b] == refs[b]["dropped"] and rejected[b] >= 100


def test_gated_second_frame_sees_nothing_of_the_first():
  B, H, W, s = 2, 23, 524, 2
  cam = _camera(H, W)
  proj = DepthProjector(H, W, cam, batch=B, pyramid_scale=s, device=DEV)
  rgb = np.random.RandomState(6).rand(B, 3, H, W).astype(F)
  for i, cmin in enumerate((0.4, 0.9, 0.1)):
    disp = _scene(B, H, W, s, seed=20 + i)
    valid = pr.points(disp, _consts(cam, s), s)["valid"]
    conf, _ = _given_conf(B, H >> s, W >> s, valid, seed=30 + i, conf_min=F(cmin))
    cloud = run_gated(proj, torch.from_numpy(disp).to(DEV), torch.from_numpy(rgb).to(DEV), torch.from_numpy(conf).to(DEV), F(cmin))
    check_gated(proj, cloud, disp, rgb, conf, F(cmin), cam, s)
  # a smaller batch, and an ungated frame, through the same buffers
  disp = _scene(1, H, W, s, seed=40)
  conf = np.random.RandomState(41).rand(1, H >> s, W >> s).astype(F)
  cloud = run_gated(proj, torch.from_numpy(disp).to(DEV), None, torch.from_numpy(conf).to(DEV), 0.5)
  check_gated(proj, cloud, disp, None, conf, 0.5, cam, s)
  plain = proj.voxel_cloud(torch.from_numpy(disp).to(DEV))
  assert plain.rejected is None
  want = pr.voxel_cloud(pr.points(disp, _consts(cam, s), s), 0, 0.15)
  assert int(plain.n[0]) == want["n"]


def test_gated_call_in_a_captured_graph():
  B, H, W, s = 2, 23, 524, 2
  cam = _camera(H, W)
  proj = DepthProjector(H, W, cam, batch=B, pyramid_scale=s, device=DEV)
  disp = _scene(B, H, W, s, seed=50)
  valid = pr.points(disp, _consts(cam, s), s)["valid"]
  confs = [_given_conf(B, H >> s, W >> s, valid, seed=60 + i)[0] for i in range(2)]
  rgb = np.random.RandomState(8).rand(B, 3, H, W).astype(F)
  s_disp, s_rgb, s_conf = (torch.from_numpy(a).to(DEV) for a in (disp, rgb, confs[0]))
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    run_gated(proj, s_disp, s_rgb, s_conf, CONF_MIN)        # warm-up outside the capture
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):     # one stream: a linear graph
    cloud = run_gated(proj, s_disp, s_rgb, s_conf, CONF_MIN)
  for conf in confs + [confs[0]]:                           # rejected is overwritten on every replay, never accumulated
    s_conf.copy_(torch.from_numpy(conf))
    graph.replay()
    torch.cuda.synchronize()
    check_gated(proj, cloud, disp, rgb, conf, CONF_MIN, cam, s)
  # conf_min is an argument of the launch: a new one needs a new capture
  graph2 = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph2, stream=side, capture_error_mode="thread_local"):
    cloud = run_gated(proj, s_disp, s_rgb, s_conf, F(0.75))
  s_conf.copy_(torch.from_numpy(confs[1]))
  graph2.replay()
  torch.cuda.synchronize()
  check_gated(proj, cloud, disp, rgb, confs[1], F(0.75), cam, s)


def test_gate_errors_return_before_any_launch():
  B, H, W, s = 1, 23, 524, 2
  cam = _camera(H, W)
  proj = DepthProjector(H, W, cam, batch=B, pyramid_scale=s, device=DEV)
  disp = torch.from_numpy(_scene(B, H, W, s, seed=70)).to(DEV)
  conf = torch.rand(B, H >> s, W >> s, device=DEV)
  cloud = run_gated(proj, disp, None, conf, 0.5)
  torch.cuda.synchronize()
  keep = (cloud.records, cloud.voxel, cloud.count, cloud.n, cloud.dropped, cloud.rejected, proj._depth, proj._xyz)
  before = [t.clone() for t in keep]
  lib = nat.load()
  for c, cmin, word in ((None, 0.5, b"conf is required"), (nat.ptr(conf), float("nan"), b"NaN")):
    assert lib.as_disp_to_points_gated(nat.ptr(disp), None, c, cmin, B, H, W, s, ctypes.byref(proj._cam), nat.ptr(proj._depth), None, 0.15,
                                       nat.ptr(proj._table), proj.slots, nat.ptr(proj._rejected), nat.stream()) == -1
    assert word in lib.as_last_error()
  assert lib.as_disp_to_points_gated(nat.ptr(disp), None, nat.ptr(conf), 0.5, B, H, W, s, ctypes.byref(proj._cam), None, None, 0.15,
                                     nat.ptr(proj._table), 512, nat.ptr(proj._rejected), nat.stream()) == -1
  assert b"slots" in lib.as_last_error()
  torch.cuda.synchronize()
  assert all(torch.equal(bits(a), bits(b)) for a, b in zip(before, keep))            # nothing ran
  with pytest.raises(ValueError, match="go together"):
    proj.voxel_cloud(disp, confidence=conf)
  with pytest.raises(ValueError, match="go together"):
    proj.organized(disp, conf_min=0.5)
  with pytest.raises(RuntimeError, match="no CPU path"):
    proj.voxel_cloud(disp, confidence=conf.cpu(), conf_min=0.5)
  with pytest.raises(RuntimeError, match="confidence has shape"):
    proj.voxel_cloud(disp, confidence=torch.cat([conf, conf]), conf_min=0.5)
  with pytest.raises(RuntimeError, match="contiguous"):
    proj.voxel_cloud(disp, confidence=conf.transpose(1, 2), conf_min=0.5)
  torch.cuda.synchronize()
  assert all(torch.equal(bits(a), bits(b)) for a, b in zip(before, keep))
  run_gated(proj, disp, None, conf, 0.5)                    # and the table was left clean
  torch.cuda.synchronize()
  assert all(torch.equal(a, b) for a, b in zip(before[3:6], keep[3:6]))               # n, dropped, rejected: the same frame again


# ================================================================================================= DepthProjector on the model's logits
def test_projector_gates_the_models_cloud_by_its_own_confidence():
  from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
  from adaptive_stereo.utils import synthetic as syn
  H, W, k = 96, 256, 4
  fnet, snet = FeatureExtractorNetwork(k), StereoNet(k, 1, 0, maxdisp=192)
  fnet.load_state_dict(syn.synthetic_state_dict(fnet.state_dict(), seed=123))
  snet.load_state_dict(syn.synthetic_state_dict(snet.state_dict(), seed=123, logit_gain=20.0))
  fnet, snet = fnet.to(DEV).eval(), snet.to(DEV).eval()
  left, right = (t.to(DEV) for t in syn.stereo_pair(1, H, W, seed=1))
  with torch.no_grad():
    out = snet(left, fnet(left), fnet(right), "l", output_cost_volume=True)
  cv = out["cost_volume_l/4"]
  assert tuple(cv.shape) == (1, 12, 6, 16)
  maps = conf_mod.disparity_confidence(cv)                 # the output as it is
  s = cr.stage(cv.detach().cpu().numpy())
  check_maps(dict(pmax=maps["pmax"], cent=maps["entropy"], mass=maps["mass"]), s, "model logits")
  disp = out["pred_disp_l/0"].detach().contiguous()
  left = left.contiguous()
  cam = StereoCamera(0.5885 * W, 1.9501 * H, 0.4972 * W, 0.4972 * H, 0.54)
  proj = DepthProjector(H, W, cam, batch=1, pyramid_scale=2, device=DEV)
  conf = maps["mass"]
  proj.voxel_cloud(disp, left, confidence=conf, conf_min=0.0)
  level = proj.confidence_level.cpu().numpy()              # the library's OWN up-sampled confidence: its arithmetic is pinned elsewhere
  assert level.shape == (1, 1, 24, 64) and np.isfinite(level).all()
  want = torch.empty(1, 1, 24, 64, device=DEV)
  nat.call("as_upsample_bilinear_fwd", nat.ptr(conf), 1, 6, 16, nat.ptr(want), 24, 64, 1.0, nat.stream())
  assert np.array_equal(_np_bits(level), _np_bits(want.cpu().numpy()))
  conf_min = float(np.median(level))                       # a gate that decides: half of the pixels on either side
  torch.cuda.synchronize()
  allocs = torch.cuda.memory_stats()["allocation.all.allocated"]
  in_use = torch.cuda.memory_allocated()
  cloud = proj.voxel_cloud(disp, left, confidence=conf.unsqueeze(1), conf_min=conf_min)
  xyz, depth = proj.organized(disp, confidence=conf, conf_min=conf_min)
  assert torch.cuda.memory_stats()["allocation.all.allocated"] == allocs and torch.cuda.memory_allocated() == in_use, "a call allocated"
  host_disp, host_left = disp.cpu().numpy(), left.cpu().numpy()
  p = pr.points(host_disp, _consts(cam, 2), 2)
  q, rejected = cr.gate(p, level[:, 0], conf_min)
  assert proj.rejected.tolist() == rejected.tolist() and 0 < rejected[0] < p["valid"].sum()
  assert np.array_equal(_np_bits(xyz.cpu().numpy()), _np_bits(pr.organized(q)))
  # organized() ran last and left the table alone: the cloud of the call before it is still in the record buffers
  ref = pr.voxel_cloud(q, 0, 0.15, pr.colour_bytes(host_left, 2))
  g = cloud.trim()[0]
  assert int(cloud.n[0]) == ref["n"] >= 5 and g["dropped"] == ref["dropped"] and cloud.rejected.tolist() == rejected.tolist()
  vox, cnt, rec = pr.sort_cloud(g["voxel"].cpu().numpy(), g["count"].cpu().numpy(), g["records"].cpu().numpy())
  assert np.array_equal(vox, ref["voxel"]) and np.array_equal(cnt, ref["count"])
  assert np.array_equal(rec[:, :3], _np_bits(ref["xyz"])) and np.array_equal(rec[:, 3].view(np.uint32), ref["rgb"])
  ungated = pr.voxel_cloud(p, 0, 0.15)
  assert ref["count"].sum() < ungated["count"].sum()
  with pytest.raises(ValueError, match="go together"):
    proj.voxel_cloud(disp, left, confidence=conf)
  with pytest.raises(ValueError, match="go together"):
    proj.voxel_cloud(disp, left, conf_min=0.5)
  # without a confidence the call is today's
  plain = proj.voxel_cloud(disp, left)
  assert plain.rejected is None and int(plain.n[0]) == pr.voxel_cloud(p, 0, 0.15, pr.colour_bytes(host_left, 2))["n"]


# ================================================================================================= as_sparsification
def run_bins(key, pred, gt, K, lo=0.0, scale=None, tau=3.0, into=None):
  """as_sparsification on host arrays -> (Guarded ints [count | bad | skipped], Guarded abs_err); `into` accumulates further"""
  scale = float(cr.bin_scale(K, 0, 1)) if scale is None else scale
  if into is None:
    gi, ge = Guarded(1, 2 * K + 1, torch.int64), Guarded(1, K, torch.float64)
    gi.views[0].zero_(); ge.views[0].zero_()
  else:
    gi, ge = into
  d = [torch.from_numpy(np.ascontiguousarray(a, dtype=F)).to(DEV) for a in (key, pred, gt)]
  base = gi.views[0].data_ptr()
  nat.call("as_sparsification", nat.ptr(d[0]), nat.ptr(d[1]), nat.ptr(d[2]), d[0].numel(), lo, scale, K, tau, nat.c_vp(base),
           nat.c_vp(base + 8 * K), nat.ptr(ge.views[0]), nat.c_vp(base + 16 * K), nat.stream())
  torch.cuda.synchronize()
  assert gi.guards_intact() and ge.guards_intact(), "a write outside the outputs"
  return gi, ge


def check_bins(gi, ge, want, n, K, what):
  ints, err = gi.views[0].cpu().numpy(), ge.views[0].cpu().numpy()
  assert ints[:K].tolist() == want["count"].tolist(), "%s: count" % what
  assert ints[K:2 * K].tolist() == want["bad"].tolist(), "%s: bad" % what
  assert int(ints[2 * K]) == want["skipped"], "%s: skipped %d, reference %d" % (what, int(ints[2 * K]), want["skipped"])
  gap, bound = np.abs(err - want["abs_err"]), cr.abs_err_bound(n, want["abs_err"])
  with np.errstate(all="ignore"):
    worst = float(np.where(gap == 0, 0.0, gap / bound).max())
  print("%s: abs_err worst |err| / bound %.3g (largest gap %.3g)" % (what, worst, gap.max()))
  assert (gap <= bound).all(), "%s: abs_err off by %s at most, bound %s" % (what, gap.max(), bound[np.argmax(gap)])


@pytest.mark.parametrize("K", cr.SPARSE_K)
@pytest.mark.parametrize("n", cr.SPARSE_N)
def test_bins_exact_counts_and_bounded_sums(n, K):
  key, pred, gt = cr.sparsify_case(n, K)
  want = cr.sparsify_loop(key, pred, gt, 0.0, cr.bin_scale(K, 0, 1), K, 3.0)
  gi, ge = run_bins(key, pred, gt, K)
  check_bins(gi, ge, want, n, K, "n %d K %d" % (n, K))


def test_bins_at_every_edge():
  K = 256
  edges = (np.arange(K + 1, dtype=np.float64) / K).astype(F)
  key = np.concatenate([edges, cr._below(edges), np.array([-0.25, 1.5, np.inf, -np.inf, np.nan], F)])
  gt = np.full(key.size, 10.0, F)
  pred = np.full(key.size, 13.0, F)                        # err == tau: not bad
  pred[::3] = np.nextafter(F(13.0), F(14.0), dtype=F)      # one ulp beyond: bad
  want = cr.sparsify_loop(key, pred, gt, 0.0, F(K), K, 3.0)
  assert want["count"].min() >= 2 and want["skipped"] == 1 and 0 < want["bad"].sum() < want["count"].sum()
  check_bins(*run_bins(key, pred, gt, K), want=want, n=key.size, K=K, what="edges")
  # another lo and a scale that is not a power of two
  lo, hi, K = -2.5, 7.5, 3
  key = (lo + (hi - lo) * np.random.RandomState(1).rand(500)).astype(F)
  want = cr.sparsify_loop(key, pred[:500], gt[:500], lo, cr.bin_scale(K, lo, hi), K, 3.0)
  check_bins(*run_bins(key, pred[:500], gt[:500], K, lo=lo, scale=float(cr.bin_scale(K, lo, hi))), want=want, n=500, K=K, what="lo -2.5")


def test_collector_accumulates_replays_and_draws_the_curve():
  K, n = 256, 4099
  parts = [cr.sparsify_case(n, K, seed=i) for i in range(3)]
  loops = [cr.sparsify_loop(k, p, g, 0.0, cr.bin_scale(K, 0, 1), K, 3.0) for k, p, g in parts]
  col = conf_mod.SparsificationCollector(bins=K, device=DEV)
  dev = [[torch.from_numpy(a).to(DEV) for a in part] for part in parts]
  col.add(*dev[0])
  before = torch.cuda.memory_allocated()
  col.add(*[t.reshape(1, -1) for t in dev[1]])             # any shape
  assert torch.cuda.memory_allocated() == before, "add() allocated"
  got = col.counts()

  def total(idx):
    terms = [loops[i] for i in idx]
    return dict(count=sum(t["count"] for t in terms), bad=sum(t["bad"] for t in terms), skipped=sum(t["skipped"] for t in terms),
                abs_err=np.array([math.fsum(float(t["abs_err"][k]) for t in terms) for k in range(K)]))

  def check(got, want, calls):
    assert got["count"].tolist() == want["count"].tolist() and got["bad"].tolist() == want["bad"].tolist()
    assert got["skipped"] == want["skipped"]
    # the reference sum of sums is itself rounded per call: one more term per call
    assert (np.abs(got["abs_err"] - want["abs_err"]) <= cr.abs_err_bound(calls * (n + 1), want["abs_err"])).all()
  check(got, total([0, 1]), 2)
  # the curve of the device counts against the plain-loop curve of the reference counts
  want = total([0, 1])
  for remove in ("low", "high"):
    a, b = col.curve(remove), cr.curve_loop(want["count"], want["bad"], want["abs_err"], remove)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])                 # integers over integers
    assert (np.abs(a[1] - b[1]) <= (2 * n + K + 4) * 2.0 ** -53 * b[1]).all()     # the bins' bound + K additions + the quotient
  assert conf_mod.ause(col.curve("low"), col.curve("low")) == 0.0
  col.reset()
  torch.cuda.synchronize()
  zero = col.counts()
  assert zero["count"].sum() == 0 and zero["bad"].sum() == 0 and zero["skipped"] == 0 and zero["abs_err"].sum() == 0
  # a captured add appends on every replay
  static = [t.clone() for t in dev[0]]
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    col.add(*static)                                       # warm-up outside the capture
  torch.cuda.synchronize()
  col.reset()
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):     # one stream: a linear graph
    col.add(*static)
  for part in dev:
    for dst, src in zip(static, part):
      dst.copy_(src)
    graph.replay()
  torch.cuda.synchronize()
  check(col.counts(), total([0, 1, 2]), 3)
  with pytest.raises(RuntimeError, match="no CPU path"):
    col.add(*[t.cpu() for t in dev[0]])
  with pytest.raises(RuntimeError, match="contiguous fp32"):
    col.add(dev[0][0].double(), dev[0][1], dev[0][2])
  with pytest.raises(RuntimeError, match="contiguous fp32"):
    col.add(dev[0][0][:-1], dev[0][1], dev[0][2])


def test_bins_errors_return_before_any_launch():
  lib = nat.load()
  K = 4
  gi, ge = Guarded(1, 2 * K + 1, torch.int64), Guarded(1, K, torch.float64)
  x = torch.ones(8, device=DEV)
  base = gi.views[0].data_ptr()

  def call(key=nat.ptr(x), n=8, lo=0.0, scale=4.0, K=K, tau=3.0, count=nat.c_vp(base), skipped=nat.c_vp(base + 16 * K)):
    return lib.as_sparsification(key, nat.ptr(x), nat.ptr(x), n, lo, scale, K, tau, count, nat.c_vp(base + 8 * K), nat.ptr(ge.views[0]),
                                 skipped, nat.stream())
  for kw in (dict(key=None), dict(skipped=None), dict(n=0), dict(n=-3), dict(K=0), dict(K=1025), dict(scale=0.0), dict(scale=-1.0),
             dict(scale=float("inf")), dict(scale=float("nan")), dict(lo=float("nan")), dict(lo=float("inf")), dict(tau=float("nan")),
             dict(count=nat.c_vp(base + 4))):
    assert call(**kw) == -1, kw
  torch.cuda.synchronize()
  assert bool((gi.raw == SENTINEL).all()) and bool((ge.raw == SENTINEL).all())
  assert call() == 0                                       # and the same call with good arguments runs
  torch.cuda.synchronize()
  assert gi.guards_intact() and ge.guards_intact()
