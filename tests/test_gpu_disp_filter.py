"""csrc/disp_filter.hip (as_disp_edge_check, as_disp_speckle) and adaptive_stereo.disp_filter on the GPU, bit for bit against
tests/disp_filter_ref.py (pinned on the CPU by tests/test_disp_filter_ref_cpu.py).  Every output is integer or a selected float,
so every comparison is exact.  Every output is written between sentinel guards, as tests/test_gpu_lr_consistency.py does.

The kernels work on tiles of DF_ROWS = 4 rows x DF_SPAN = 256 columns, a wave on DF_WAVE = 64 consecutive pixels of a row;
disp_filter_ref.SHAPES and the patterns place their boundaries by these.  The union-find patterns (checkerboard, comb, serpentine,
spiral, U, one component) are the orders of merging a random map does not produce."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import confidence_ref as cr
import disp_filter_ref as df
import lr_consistency_ref as lr
import pointcloud_ref as pr
from dataset_fixture import make_tree
from test_gpu_end_to_end import build
from adaptive_stereo import _native as nat
from adaptive_stereo import consistency as cons
from adaptive_stereo import disp_filter as dfm
from adaptive_stereo.pointcloud import DepthProjector, StereoCamera
from adaptive_stereo.utils import synthetic as syn
from guarded_buffers import DEV, F, GUARD, SENTINEL, SENTINEL_I32, SENTINEL_U8, dev, same_bits

EDGE_OUTS = ("code", "valid", "jump", "counts")
SPECKLE_OUTS = ("label", "size", "code", "valid", "counts")
SHAPE_IDS = ["x".join(map(str, s)) for s in df.SHAPES]
PATTERN_SHAPES = [(1, 2 * df.DF_ROWS + 1, df.DF_SPAN + 7), (2, df.DF_ROWS + 2, 2 * df.DF_WAVE + 3)]
MODEL_FILTER = dict(tol_abs=0.5, tol_rel=0.0, max_diff=0.25, max_size=30)      # thresholds at which the model's maps show every code


class Guarded(object):
  """one buffer of n elements inside a sentinel-filled allocation, GUARD elements on either side"""

  def __init__(self, n, dtype, sentinel):
    self.sentinel = sentinel
    self.raw = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)
    self.view = self.raw[GUARD:GUARD + n]

  def guards_intact(self):
    return bool((self.raw[:GUARD] == self.sentinel).all()) and bool((self.raw[-GUARD:] == self.sentinel).all())

  def untouched(self):
    return bool((self.raw == self.sentinel).all())


def _buffers(B, n):
  return dict(code=Guarded(n, torch.uint8, SENTINEL_U8), valid=Guarded(n, torch.float32, SENTINEL),
              jump=Guarded(n, torch.float32, SENTINEL), label=Guarded(n, torch.int32, SENTINEL_I32),
              size=Guarded(n, torch.int32, SENTINEL_I32), counts=Guarded(B * df.CODES, torch.int32, SENTINEL_I32))


def _collect(g, names, which, shape):
  B, H, W = shape
  torch.cuda.synchronize()
  for k in names:
    assert g[k].guards_intact(), "a write outside %s" % k
    if k not in which:
      assert g[k].untouched(), "%s was not requested and was written" % k
  return {k: g[k].view.reshape((B, df.CODES) if k == "counts" else (B, 1, H, W)) for k in which}


def run_edge(disp, code_in, tol, which=EDGE_OUTS):
  """as_disp_edge_check on device maps [B,1,H,W] -> {name: device tensor} of the requested outputs"""
  B, _, H, W = disp.shape
  g = _buffers(B, B * H * W)
  nat.call("as_disp_edge_check", nat.ptr(disp), nat.ptr(code_in), B, H, W, tol[0], tol[1],
           *([nat.ptr(g[k].view) if k in which else None for k in EDGE_OUTS] + [nat.stream()]))
  return _collect(g, EDGE_OUTS, which, (B, H, W))


def run_speckle(disp, code_in, max_diff, max_size, which=SPECKLE_OUTS):
  B, _, H, W = disp.shape
  g = _buffers(B, B * H * W)
  nat.call("as_disp_speckle", nat.ptr(disp), nat.ptr(code_in), B, H, W, max_diff, max_size,
           *([nat.ptr(g[k].view) if k in which else None for k in SPECKLE_OUTS] + [nat.stream()]))
  return _collect(g, SPECKLE_OUTS, which, (B, H, W))


def assert_same(got, want, names, what=""):
  for k in names:
    if not same_bits(got[k], want[k]):
      g = got[k].cpu().numpy()
      bad = np.argwhere(g.view(np.uint32) != want[k].view(np.uint32) if g.dtype == F else g != want[k])
      raise AssertionError("%s %s: %d elements differ, first %s: got %s, want %s"
                           % (what, k, len(bad), bad[:4].tolist(), g[tuple(bad[0])], want[k][tuple(bad[0])]))


@pytest.fixture(scope="module")
def cases():
  """the random inputs and the restatement's answers of every shape, computed once and left unchanged"""
  out = {}
  for shape in df.SHAPES:
    d, c = df.random_case(shape)
    out[shape] = dict(disp=d, code_in=c,
                      edge={(tol, coded): df.edge_check(d, c if coded else None, *tol) for tol in df.TOLS for coded in (False, True)},
                      speckle={(sp, coded): df.speckle(d, c if coded else None, *sp) for sp in df.SPECKLES for coded in (False, True)})
  return out


# ================================================================================================= as_disp_edge_check
@pytest.mark.parametrize("tol", df.TOLS, ids=lambda t: "tol%g_%g" % t)
@pytest.mark.parametrize("shape", df.SHAPES, ids=SHAPE_IDS)
def test_edge_check_bit_for_bit(cases, shape, tol):
  case = cases[shape]
  disp, code_in = dev(case["disp"]), dev(case["code_in"])
  for coded in (False, True):
    together = run_edge(disp, code_in if coded else None, tol)
    assert_same(together, case["edge"][(tol, coded)], EDGE_OUTS, "coded %s" % coded)
  for k in EDGE_OUTS:                                                # each output alone: the same bits, nothing else written
    alone = run_edge(disp, code_in, tol, which=(k,))
    assert torch.equal(alone[k].view(torch.uint8), together[k].view(torch.uint8)), "alone " + k
  assert same_bits(disp, case["disp"]) and same_bits(code_in, case["code_in"]), "an input was written"


@pytest.mark.parametrize("shape", PATTERN_SHAPES + [(2, 2, 1242)], ids=lambda s: "x".join(map(str, s)))
def test_edge_check_halo_across_every_tile_and_wave_boundary(shape):
  """steps of 3 exactly at the wave boundaries in x and the tile boundaries in y (between two workgroups' rows): a pixel is
  flagged only through a neighbour that another wave or workgroup holds (the CPU test pins which pixels those are)"""
  d = df.tile_steps(shape)
  want = df.edge_check(d, None, 1.0, 0.0)
  assert (want["code"] == 5).any() and (want["code"] == 0).any()
  assert_same(run_edge(dev(d), None, (1.0, 0.0)), want, EDGE_OUTS)
  assert_same(run_edge(dev(d), None, (float("inf"), 0.0)), df.edge_check(d, None, np.inf, 0.0), EDGE_OUTS, "tol_abs inf")
  assert_same(run_edge(dev(d), None, (0.0, float("inf"))), df.edge_check(d, None, 0.0, np.inf), EDGE_OUTS, "tol_rel inf")


# ================================================================================================= as_disp_speckle
@pytest.mark.parametrize("sp", df.SPECKLES, ids=lambda s: "diff%g_size%d" % s)
@pytest.mark.parametrize("shape", df.SHAPES, ids=SHAPE_IDS)
def test_speckle_bit_for_bit(cases, shape, sp):
  case = cases[shape]
  disp, code_in = dev(case["disp"]), dev(case["code_in"])
  for coded in (False, True):
    together = run_speckle(disp, code_in if coded else None, *sp)
    assert_same(together, case["speckle"][(sp, coded)], SPECKLE_OUTS, "coded %s" % coded)
  required = ("label", "size")
  for k in ("code", "valid", "counts"):                              # each optional output alone beside the two required ones
    alone = run_speckle(disp, code_in, *sp, which=required + (k,))
    for name in required + (k,):
      assert torch.equal(alone[name].view(torch.uint8), together[name].view(torch.uint8)), "alone %s: %s" % (k, name)
  bare = run_speckle(disp, code_in, *sp, which=required)
  assert torch.equal(bare["label"], together["label"]) and torch.equal(bare["size"], together["size"])
  assert same_bits(disp, case["disp"]) and same_bits(code_in, case["code_in"]), "an input was written"


def test_speckle_every_usable_pair_joined(cases):
  case = cases[(2, 5, 63)]
  want = df.speckle(case["disp"], None, np.inf, 7)
  assert_same(run_speckle(dev(case["disp"]), None, float("inf"), 7), want, SPECKLE_OUTS)
  none = run_speckle(dev(case["disp"]), None, 0.0, 0)                # max_diff 0 joins equal neighbours; max_size 0 rejects nothing
  assert_same(none, df.speckle(case["disp"], None, 0.0, 0), SPECKLE_OUTS)
  assert not bool((none["code"] == 6).any())


@pytest.mark.parametrize("shape", PATTERN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", sorted(df.PATTERNS))
def test_speckle_union_find_patterns(name, shape):
  d = df.PATTERNS[name](shape)
  want = df.speckle(d, None, 1.0, 5)
  got = run_speckle(dev(d), None, 1.0, 5)
  assert_same(got, want, SPECKLE_OUTS, name)
  if name != "checkerboard":                                         # one component an image: its first pixel is pixel 0
    kept = torch.from_numpy(~np.isnan(d)).to(DEV)
    assert bool((got["label"][kept] == 0).all()) and bool((got["size"][kept] == int(kept[0].sum())).all())


def test_speckle_one_component_covers_the_product_image():
  """465750 pixels count themselves on one counter: one integer atomic per wave"""
  B, H, W = 1, 375, 1242
  d = torch.full((B, 1, H, W), 12.5, device=DEV)
  got = run_speckle(d, None, 1.0, H * W - 1)
  assert bool((got["size"] == H * W).all()) and bool((got["label"] == 0).all()) and bool((got["code"] == 0).all())
  assert got["counts"].tolist() == [[H * W, 0, 0, 0, 0, 0, 0]]
  got = run_speckle(d, None, 1.0, H * W, which=("label", "size", "code"))
  assert bool((got["code"] == 6).all()) and bool((got["size"] == H * W).all())


def test_speckle_same_image_twice_in_a_batch(cases):
  one = cases[(1, 5, df.DF_SPAN + 1)]["disp"]
  twice = np.concatenate([one, one])
  got = run_speckle(dev(twice), None, 1.0, 3)
  assert_same(got, df.speckle(twice, None, 1.0, 3), SPECKLE_OUTS)
  for k in ("label", "size", "code"):
    assert torch.equal(got[k][0], got[k][1]), k
  assert int(got["label"].max()) < one.size


# ================================================================================================= DisparityFilter: state, replay
def _assert_filter(filt, want_e, want_s, what=""):
  assert_same(dict(code=filt.code, valid=filt.valid, label=filt.label, size=filt.size, counts=filt.counts), want_s,
              SPECKLE_OUTS, what)
  assert same_bits(filt.jump, want_e["jump"]), what + " jump"


def test_two_calls_in_a_row_overwrite_counts_and_working_state(cases):
  shape = (2, 5, 63)
  B, H, W = shape
  d0, c0 = cases[shape]["disp"], cases[shape]["code_in"]
  d1, c1 = df.random_case(shape, seed=5)
  flt = dfm.DisparityFilter(H, W, batch=B, tol_abs=1.0, max_diff=1.0, max_size=3, device=DEV)
  want0, want1 = df.disparity_filter(d0, c0, 1.0, 0.0, 1.0, 3), df.disparity_filter(d1, None, 1.0, 0.0, 1.0, 3)
  assert not np.array_equal(want0[1]["counts"], want1[1]["counts"])
  _assert_filter(flt(dev(d0), dev(c0)), *want0, what="first")
  _assert_filter(flt(dev(d1)), *want1, what="second")                # other data, the same buffers: nothing accumulates
  assert np.array_equal(flt.fractions(), want1[1]["counts"].astype(np.float64) / (H * W))
  _assert_filter(flt(dev(d0), dev(c0)), *want0, what="third")
  e = flt.edges(dev(d1), dev(c1))                                    # the two halves on their own
  assert e.label is None and e.size is None
  assert_same(e._asdict(), df.edge_check(d1, c1, 1.0, 0.0), EDGE_OUTS, "edges")
  s = flt.speckles(dev(d1), dev(c1))
  assert s.jump is None
  assert_same(s._asdict(), df.speckle(d1, c1, 1.0, 3), SPECKLE_OUTS, "speckles")
  with pytest.raises(RuntimeError, match=r"\(2, 1, 5, 63\).*\(2, 1, 5, 4\)"):
    flt(torch.zeros(B, 1, H, 4, device=DEV))
  with pytest.raises(RuntimeError, match="contiguous fp32"):
    flt(dev(d0).double())
  with pytest.raises(RuntimeError, match="uint8"):
    flt(dev(d0), dev(d0))


def test_graph_replay_on_a_second_input_equals_eager(cases):
  shape = (1, 5, df.DF_SPAN + 1)
  B, H, W = shape
  d0, c0 = cases[shape]["disp"], cases[shape]["code_in"]
  d1, c1 = df.random_case(shape, seed=9)
  flt = dfm.DisparityFilter(H, W, batch=B, tol_abs=0.5, tol_rel=0.0625, max_diff=0.25, max_size=40, device=DEV)
  eager = [t.clone() for t in flt(dev(d1), dev(c1))]
  static_d, static_c = dev(d0), dev(c0)
  side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    flt(static_d, static_c)                                          # warm-up on the capturing stream
  torch.cuda.synchronize()
  with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
    result = flt(static_d, static_c)
  static_d.copy_(dev(d1)); static_c.copy_(dev(c1))
  graph.replay()
  torch.cuda.synchronize()
  for name, a, b in zip(result._fields, result, eager):
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "%s differs between replay and eager" % name
  _assert_filter(result, *df.disparity_filter(d1, c1, 0.5, 0.0625, 0.25, 40), what="replay")
  graph.replay()                                                     # and again: the working arrays clean themselves
  torch.cuda.synchronize()
  for name, a, b in zip(result._fields, result, eager):
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "%s differs on the second replay" % name


# ================================================================================================= refusals
def test_refusals_set_the_error_and_launch_nothing():
  lib = nat.load()
  B, H, W = 1, 2, 8
  n = B * H * W
  x = torch.zeros(B, 1, H, W, device=DEV)
  cin = torch.zeros(B, 1, H, W, dtype=torch.uint8, device=DEV)
  g = _buffers(B, n)
  o = {k: nat.ptr(v.view) for k, v in g.items()}
  px, pc, s = nat.ptr(x), nat.ptr(cin), nat.stream()
  nan = float("nan")
  refused = [
    ("as_disp_edge_check", (None, pc, B, H, W, 1.0, 0.0, o["code"], o["valid"], o["jump"], o["counts"], s), "null"),
    ("as_disp_edge_check", (px, pc, B, 0, W, 1.0, 0.0, o["code"], o["valid"], o["jump"], o["counts"], s), "shape"),
    ("as_disp_edge_check", (px, pc, 65536, H, W, 1.0, 0.0, o["code"], o["valid"], o["jump"], o["counts"], s), "65535"),
    ("as_disp_edge_check", (px, pc, B, H, W, nan, 0.0, o["code"], o["valid"], o["jump"], o["counts"], s), "tol_abs"),
    ("as_disp_edge_check", (px, pc, B, H, W, 1.0, -0.5, o["code"], o["valid"], o["jump"], o["counts"], s), "tol_rel"),
    ("as_disp_edge_check", (px, pc, B, H, W, 1.0, 0.0, None, None, None, None, s), "no output"),
    ("as_disp_edge_check", (px, pc, B, H, W, 1.0, 0.0, o["code"], px, o["jump"], o["counts"], s), "alias"),
    ("as_disp_edge_check", (px, pc, B, H, W, 1.0, 0.0, pc, o["valid"], o["jump"], o["counts"], s), "alias"),
    ("as_disp_edge_check", (px, pc, B, H, W, 1.0, 0.0, o["code"], o["valid"], o["valid"], o["counts"], s), "alias"),
    ("as_disp_speckle", (px, pc, B, H, W, 1.0, 3, None, o["size"], o["code"], o["valid"], o["counts"], s), "null"),
    ("as_disp_speckle", (px, pc, B, H, W, 1.0, 3, o["label"], None, o["code"], o["valid"], o["counts"], s), "null"),
    ("as_disp_speckle", (px, pc, B, H, -W, 1.0, 3, o["label"], o["size"], o["code"], o["valid"], o["counts"], s), "shape"),
    ("as_disp_speckle", (px, pc, B, H, W, nan, 3, o["label"], o["size"], o["code"], o["valid"], o["counts"], s), "max_diff"),
    ("as_disp_speckle", (px, pc, B, H, W, -1.0, 3, o["label"], o["size"], o["code"], o["valid"], o["counts"], s), "max_diff"),
    ("as_disp_speckle", (px, pc, B, H, W, 1.0, -3, o["label"], o["size"], o["code"], o["valid"], o["counts"], s), "max_size"),
    ("as_disp_speckle", (px, pc, B, H, W, 1.0, 3, o["label"], o["label"], o["code"], o["valid"], o["counts"], s), "alias"),
    ("as_disp_speckle", (px, pc, B, H, W, 1.0, 3, px, o["size"], o["code"], o["valid"], o["counts"], s), "alias"),
    ("as_disp_speckle", (px, pc, B, H, W, 1.0, 3, o["label"], o["size"], pc, o["valid"], o["counts"], s), "alias"),
    ("as_disp_speckle", (px, pc, B, H, W, 1.0, 3, o["label"], o["size"], o["code"], o["size"], o["counts"], s), "alias"),
  ]
  for name, args, word in refused:
    assert getattr(lib, name)(*args) == -1, (name, word)
    assert re.search(word, lib.as_last_error().decode()), (name, word, lib.as_last_error())
  torch.cuda.synchronize()
  assert all(v.untouched() for v in g.values()) and not bool(x.any()) and not bool(cin.any())


# ================================================================================================= on the model's own disparity
B, H, W, K, MAXDISP = 2, 83, 150, 3, 100


@pytest.fixture(scope="module")
def world():
  """the networks in eval mode and two different batches of pairs on the device (as tests/test_gpu_both_view.py builds them)"""
  fnet, snet = build(dict(k=K, s=0, maxdisp=MAXDISP, gain=200.0))
  fnet.eval(); snet.eval()
  pairs = [syn.stereo_pair(B, H, W, seed=seed, disparities=(3.0, 9.0, 14.0)[:B]) for seed in (7, 8)]
  dev_pairs = [(l.to(DEV).contiguous(), r.to(DEV).contiguous()) for l, r in pairs]
  return dict(fnet=fnet, snet=snet, dev_pairs=dev_pairs)


def check_pipeline_against_restatement(disp_l, disp_r, chk, filt, filled, note=None):
  """every decision of the chain is exact given the two disparity maps: the check, the filter on what it kept, the fill from the
  combined code, and no filled value that comes from a rejected pixel"""
  m = MODEL_FILTER
  dl = disp_l.cpu().numpy()
  want_chk = lr.lr_check(dl, disp_r.cpu().numpy(), 1.0, 0.0)
  for k in chk._fields:
    assert same_bits(getattr(chk, k), want_chk[k]), k
  want_e, want_s = df.disparity_filter(dl, want_chk["code_l"], m["tol_abs"], m["tol_rel"], m["max_diff"], m["max_size"])
  _assert_filter(filt, want_e, want_s, "pipeline")
  assert same_bits(filled, lr.lr_fill(dl, want_s["code"]))
  got, code = filled.cpu().numpy(), want_s["code"]
  for b in range(dl.shape[0]):
    for y in range(dl.shape[2]):
      kept = set(dl[b, 0, y][code[b, 0, y] == 0].view(np.uint32).tolist()) or {0}       # a row without any: 0.0
      assert set(got[b, 0, y].view(np.uint32).tolist()) <= kept, "row %d of image %d holds a value of a rejected pixel" % (y, b)
  return want_s


def test_disparity_filter_on_the_models_disparity(world):
  from adaptive_stereo.collect import stereo_forward
  left, right = world["dev_pairs"][0]
  with torch.no_grad():
    disp = stereo_forward(world["fnet"], world["snet"], left, right)["pred_disp_l/0"].float().contiguous()
  flt = dfm.DisparityFilter(H, W, batch=B, device=DEV, **MODEL_FILTER)
  filt = flt(disp)
  m = MODEL_FILTER
  want_e, want_s = df.disparity_filter(disp.cpu().numpy(), None, m["tol_abs"], m["tol_rel"], m["max_diff"], m["max_size"])
  _assert_filter(filt, want_e, want_s, "single view")
  print("codes of the model's left view, single view:", want_s["counts"].tolist())
  assert {0, 5, 6} <= set(np.unique(want_s["code"]).tolist()), "the scene exercises the filter"
  assert np.allclose(flt.fractions().sum(axis=1), 1.0)


def test_filtered_both_view_pipeline_eager_and_replayed(world):
  fnet, snet = world["fnet"], world["snet"]
  (l0, r0), (l1, r1) = world["dev_pairs"]
  plain = cons.BothViewInference(fnet, snet, H, W, batch=B)
  p_disp_l, p_disp_r, p_chk, _ = plain(l0, r0)
  p_disp_l, p_code = p_disp_l.clone(), p_chk.code_l.clone()
  both = dfm.FilteredBothViewInference(fnet, snet, H, W, batch=B, edge_tol_abs=MODEL_FILTER["tol_abs"], edge_tol_rel=MODEL_FILTER["tol_rel"],
                                       max_diff=MODEL_FILTER["max_diff"], max_size=MODEL_FILTER["max_size"])
  disp_l, disp_r, chk, filt, filled = both(l0, r0)
  torch.cuda.synchronize()
  assert torch.equal(disp_l, p_disp_l) and torch.equal(chk.code_l, p_code), "the stage changes nothing before it"
  want = check_pipeline_against_restatement(disp_l, disp_r, chk, filt, filled)
  print("codes of the model's left view after the left-right check:", want["counts"].tolist())
  assert {0, 5, 6} <= set(np.unique(want["code"]).tolist()) and len(np.unique(want["code"])) >= 4
  e = both(l1, r1)
  eager = [t.clone() for t in (e[0], e[1]) + tuple(e[2]) + tuple(e[3]) + (e[4],)]     # the buffers are overwritten by the next call
  both.capture(l0, r0)
  r = both(l1, r1)                                                   # a copy into the static inputs + one replay
  torch.cuda.synchronize()
  replayed = [r[0], r[1]] + list(r[2]) + list(r[3]) + [r[4]]
  assert len(replayed) == len(eager) == 2 + 7 + 6 + 1
  for i, (a, b) in enumerate(zip(replayed, eager)):
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "output %d differs between replay and eager" % i
  check_pipeline_against_restatement(*r)


def test_cloud_gated_by_the_filter(world):
  left, right = world["dev_pairs"][0]
  from adaptive_stereo.collect import stereo_forward
  with torch.no_grad():
    disp = stereo_forward(world["fnet"], world["snet"], left, right)["pred_disp_l/0"].float().contiguous()
  filt = dfm.DisparityFilter(H, W, batch=B, device=DEV, **MODEL_FILTER)(disp)
  cam = StereoCamera(721.5, 721.5 * 1.03, 0.37 * W + 0.3, 0.45 * H + 0.7, 0.54)
  proj = DepthProjector(H, W, cam, batch=B, pyramid_scale=0, device=DEV)
  cloud = proj.voxel_cloud(disp, left, confidence=filt.valid, conf_min=1.0)
  level = proj.confidence_level.cpu().numpy()
  assert np.array_equal(level.view(np.uint32), filt.valid.cpu().numpy().view(np.uint32)), "valid reaches the gate unchanged"
  host_disp, host_left = disp.cpu().numpy(), left.cpu().numpy()
  consts = pr.camera_constants(cam.fx, cam.fy, cam.cx, cam.cy, cam.baseline, 0)
  q, rejected = cr.gate(pr.points(host_disp, consts, 0), level[:, 0], 1.0)
  assert cloud.rejected.tolist() == rejected.tolist() and all(0 < r for r in rejected)
  got = cloud.trim()
  for b in range(B):
    ref = pr.voxel_cloud(q, b, 0.15, pr.colour_bytes(host_left, 0))
    g = got[b]
    assert int(cloud.n[b]) == ref["n"] and g["dropped"] == ref["dropped"]
    vox, cnt, rec = pr.sort_cloud(g["voxel"].cpu().numpy(), g["count"].cpu().numpy(), g["records"].cpu().numpy())
    assert np.array_equal(vox, ref["voxel"]) and np.array_equal(cnt, ref["count"])
    assert np.array_equal(rec[:, :3], np.ascontiguousarray(ref["xyz"], dtype=F).view(np.int32))
    assert np.array_equal(rec[:, 3].view(np.uint32), ref["rgb"])


def test_evaluate_model_post_filter_on_an_injected_dataset(tmp_path, capsys):
  import evaluate_model as E
  from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
  k, h, w, n = 3, 64, 96, 3
  data, splits = make_tree(str(tmp_path), "KittiStereo2015", n=n, H0=70, W0=110, seed=3)
  weights = str(tmp_path / "weights")
  os.makedirs(weights)
  fnet, snet = FeatureExtractorNetwork(k), StereoNet(k, 1, 0)
  torch.save(syn.synthetic_state_dict(fnet.state_dict(), seed=123), os.path.join(weights, "feature_net.pth"))
  torch.save(syn.synthetic_state_dict(snet.state_dict(), seed=123, logit_gain=5.0), os.path.join(weights, "stereo_net.pth"))
  args = ["--dataset_path", data, "--dataset_name", "KittiStereo2015", "--split", "tiny", "--subsplit", "train",
          "--splits_path", splits, "--load_weights_folder", weights, "--stereonet_k", str(k), "--batch_size", "2",
          "--height", str(h), "--width", str(w), "--num_workers", "0"]
  flags = ["--post_filter", "--edge_tol", "0.5", "--speckle_size", "30", "--speckle_diff", "0.25"]
  folder = os.path.join(weights, "outputs", "tiny")
  load = lambda name, i: torch.load(os.path.join(folder, name, "%04d.pt" % i))

  E.main(E.make_parser().parse_args(["--mode", "save"] + flags + args))              # single view
  assert "filter_code_l_0" in os.listdir(folder) and "lr_code_l_0" not in os.listdir(folder)
  for i in range(n):
    code, disp = load("filter_code_l_0", i), load("pred_disp_l_0", i)
    assert tuple(code.shape) == (1, h, w) and code.dtype == torch.uint8 and not code.is_cuda
    want = df.disparity_filter(disp.numpy()[None], None, 0.5, 0.0, 0.25, 30)[1]["code"][0]
    assert np.array_equal(code.numpy(), want), i

  E.main(E.make_parser().parse_args(["--mode", "save", "--lr_check"] + flags + args))  # on what the left-right check kept
  for i in range(n):
    code, lr_code, disp = load("filter_code_l_0", i), load("lr_code_l_0", i), load("pred_disp_l_0", i)
    want = df.disparity_filter(disp.numpy()[None], lr_code.numpy()[None], 0.5, 0.0, 0.25, 30)[1]["code"][0]
    assert np.array_equal(code.numpy(), want), i
    assert same_bits(load("pred_disp_l_filled_0", i), lr.lr_fill(disp.numpy(), want)), i

  capsys.readouterr()
  E.main(E.make_parser().parse_args(["--mode", "eval"] + flags + args))
  out = capsys.readouterr().out
  assert "pixels the post-filter keeps:" in out and "'kept':" in out.split("pixels the post-filter keeps:")[1]
  E.main(E.make_parser().parse_args(["--mode", "eval", "--lr_check"] + flags + args))
  assert "pixels the post-filter keeps after the left-right check:" in capsys.readouterr().out
  assert not E.make_parser().parse_args(["--mode", "save"] + args).post_filter         # default off
