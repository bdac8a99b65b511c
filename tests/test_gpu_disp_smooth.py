"""csrc/disp_smooth.hip (as_disp_wmedian) and adaptive_stereo.smooth on the GPU, bit for bit against tests/disp_smooth_ref.py
(pinned on the CPU by tests/test_disp_smooth_ref_cpu.py).  The output is a selected float and the rest integer, so every comparison
is exact.  Every output is written between sentinel guards, and an output that was not requested stays untouched.

The kernel works on tiles of DS_ROWS = 16 rows x DS_SPAN = 64 columns with a halo of the radius; disp_smooth_ref.SHAPES places its
boundaries by these.  There are two routes, one per (radius, guided) pair: the plain median at radius 1 and 2 sorts its taps in
registers, everything else bisects on the key; SETTINGS and the radius sweep run both on the same inputs."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import disp_filter_ref as df
import disp_smooth_ref as ds
import lr_consistency_ref as lr
from dataset_fixture import make_tree
from test_gpu_disp_filter import Guarded
from test_gpu_end_to_end import build
from adaptive_stereo import _native as nat
from adaptive_stereo import capture
from adaptive_stereo import disp_filter as dfm
from adaptive_stereo import sgm as sgm_mod
from adaptive_stereo import smooth
from adaptive_stereo.utils import synthetic as syn
from guarded_buffers import DEV, F, SENTINEL, SENTINEL_I32, SENTINEL_U8, dev, same_bits

OUTS = ("out", "code", "counts")
SHAPE_IDS = ["x".join(map(str, s)) for s in ds.SHAPES]
# (radius, channels of the guide or 0, fill, min_support or None for the default); 10 ** 6 is above every n
SETTINGS = [(1, 0, False, 1), (2, 0, True, None), (2, 3, True, None), (7, 1, True, 1), (3, 0, True, 10 ** 6), (4, 3, False, 1)]
SETTING_IDS = ["r%d_c%d_fill%d_ms%s" % (r, c, f, m) for r, c, f, m in SETTINGS]


def run_wmedian(disp, code_in, guide, lut, radius, fill, min_support, which=OUTS):
  """as_disp_wmedian on device tensors -> {name: device tensor} of the requested outputs"""
  B, _, H, W = disp.shape
  n = B * H * W
  g = dict(out=Guarded(n, torch.float32, SENTINEL), code=Guarded(n, torch.uint8, SENTINEL_U8),
           counts=Guarded(B * ds.COUNTS, torch.int32, SENTINEL_I32))
  nat.call("as_disp_wmedian", nat.ptr(disp), nat.ptr(code_in), nat.ptr(guide), 0 if guide is None else guide.shape[1], nat.ptr(lut),
           B, H, W, radius, int(fill), min_support, *([nat.ptr(g[k].view) if k in which else None for k in OUTS] + [nat.stream()]))
  torch.cuda.synchronize()
  for k in OUTS:
    assert g[k].guards_intact(), "a write outside %s" % k
    if k not in which:
      assert g[k].untouched(), "%s was not requested and was written" % k
  return {k: g[k].view.reshape((B, ds.COUNTS) if k == "counts" else (B, 1, H, W)) for k in which}


def assert_same(got, want, names=OUTS, what=""):
  for k in names:
    if not same_bits(got[k], want[k]):
      g = got[k].cpu().numpy()
      bad = np.argwhere(g.view(np.uint32) != want[k].view(np.uint32) if g.dtype == F else g != want[k])
      raise AssertionError("%s %s: %d elements differ, first %s: got %s, want %s"
                           % (what, k, len(bad), bad[:4].tolist(), g[tuple(bad[0])], want[k][tuple(bad[0])]))


def _min_support(radius, ms):
  return ds.default_min_support(radius) if ms is None else ms


@pytest.fixture(scope="module")
def cases():
  """the random inputs of every shape and guide depth and the restatement's answers, computed once and left unchanged"""
  out = {}
  for shape in ds.SHAPES:
    for C in (1, 3):
      d, c, g, lut = ds.random_case(shape, channels=C)
      out[(shape, C)] = dict(disp=d, code_in=c, guide=g, lut=lut, want={})
    for r, C, fill, ms in SETTINGS:
      case = out[(shape, C or 3)]
      case["want"][(r, C, fill, ms)] = ds.wmedian(case["disp"], case["code_in"], case["guide"] if C else None,
                                                  case["lut"] if C else None, r, fill, _min_support(r, ms))
  return out


# ================================================================================================= as_disp_wmedian
@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("shape", ds.SHAPES, ids=SHAPE_IDS)
def test_wmedian_bit_for_bit(cases, shape, setting):
  r, C, fill, ms = setting
  case = cases[(shape, C or 3)]
  disp, code_in = dev(case["disp"]), dev(case["code_in"])
  guide, lut = (dev(case["guide"]), dev(case["lut"])) if C else (None, None)
  want = case["want"][setting]
  together = run_wmedian(disp, code_in, guide, lut, r, fill, _min_support(r, ms))
  assert_same(together, want, what="coded")
  assert together["counts"].sum(dim=1).tolist() == [shape[1] * shape[2]] * shape[0]
  for which in (("out",), ("out", "code"), ("out", "counts")):        # the optional outputs left out: the same bits, nothing else written
    alone = run_wmedian(disp, code_in, guide, lut, r, fill, _min_support(r, ms), which=which)
    for k in which:
      assert torch.equal(alone[k].view(torch.uint8), together[k].view(torch.uint8)), "alone %s: %s" % (which, k)
  assert same_bits(disp, case["disp"]) and same_bits(code_in, case["code_in"]), "an input was written"
  if C:
    assert same_bits(guide, case["guide"]) and same_bits(lut, case["lut"]), "an input was written"


@pytest.mark.parametrize("radius", range(1, ds.MAX_RADIUS + 1))
def test_every_radius_guided_and_not_without_codes(cases, radius):
  shape = ds.ONE_TILE_PLUS
  for C in (0, 1, 3):
    case = cases[(shape, C or 3)]
    guide, lut = (case["guide"], case["lut"]) if C else (None, None)
    ms = ds.default_min_support(radius)
    want = ds.wmedian(case["disp"], None, guide, lut, radius, True, ms)
    assert_same(run_wmedian(dev(case["disp"]), None, dev(guide), dev(lut), radius, True, ms), want, what="C %d" % C)


def test_a_small_image_under_the_largest_window(cases):
  """(1, 3, 5) at radius 7: every window is the whole image"""
  case = cases[(ds.SMALL, 3)]
  for ms in (1, 4, 16):
    want = ds.wmedian(case["disp"], None, case["guide"], case["lut"], 7, True, ms)
    got = run_wmedian(dev(case["disp"]), None, dev(case["guide"]), dev(case["lut"]), 7, True, ms)
    assert_same(got, want, what="min_support %d" % ms)


@pytest.mark.parametrize("radius", (1, 2, 5))
def test_ties_signed_zeros_and_even_counts(radius):
  d = ds.ties_case(ds.ONE_TILE_PLUS, seed=radius)
  assert (ds.bits(d) == 0x80000000).any() and (ds.bits(d) == 0).any()
  for fill in (False, True):
    want = ds.wmedian(d, None, None, None, radius, fill, 2)
    assert_same(run_wmedian(dev(d), None, None, None, radius, fill, 2), want, what="fill %s" % fill)
  if radius <= 2:                                                    # both zeros are medians somewhere: their order shows
    assert (ds.bits(want["out"]) == 0x80000000).any() and (ds.bits(want["out"]) == 0).any()


def test_the_table_of_a_real_sigma_and_a_constant_map(cases):
  case = cases[(ds.TWO_TILES_PLUS, 3)]
  lut = ds.weight_table(0.08, 3)
  want = ds.wmedian(case["disp"], case["code_in"], case["guide"], lut, 3, True, 25)
  assert_same(run_wmedian(dev(case["disp"]), dev(case["code_in"]), dev(case["guide"]), dev(lut), 3, True, 25), want)
  flat = np.full((1, 1, 20, 70), F(7.25), dtype=F)
  got = run_wmedian(dev(flat), None, None, None, 7, False, 1)
  assert same_bits(got["out"], flat) and got["counts"].tolist() == [[1400, 0, 0, 0]] and not bool(got["code"].any())


# ================================================================================================= DisparitySmoother
def test_smoother_matches_the_restatement_and_overwrites_its_state(cases):
  shape = ds.TWO_TILES_PLUS
  B, H, W = shape
  case = cases[(shape, 3)]
  d1, c1, g1, _ = ds.random_case(shape, seed=4)
  sm = smooth.DisparitySmoother(H, W, batch=B, radius=2, sigma_color=0.1, fill=True, device=DEV)
  assert np.array_equal(sm.weight_table(), ds.weight_table(0.1, 3)) and sm.min_support == 13
  lut = sm.weight_table()
  for d, c, g in ((case["disp"], case["code_in"], case["guide"]), (d1, None, g1), (case["disp"], case["code_in"], case["guide"])):
    r = sm(dev(d), dev(g), dev(c))
    want = ds.wmedian(d, c, g, lut, 2, True, 13)
    assert_same(dict(out=r.disp, code=r.code, counts=r.counts), want)
    assert np.array_equal(sm.fractions(), want["counts"].astype(np.float64) / (H * W))
  plain = smooth.DisparitySmoother(H, W, batch=B, radius=1, device=DEV)
  assert (plain.weight_table() == 1).all()
  r = plain(dev(d1))
  assert_same(dict(out=r.disp, code=r.code, counts=r.counts), ds.wmedian(d1, None, None, None, 1, False, 5))
  with pytest.raises(RuntimeError, match="takes no guide"):
    plain(dev(d1), dev(g1))
  with pytest.raises(RuntimeError, match="needs a guide"):
    sm(dev(d1))
  with pytest.raises(RuntimeError, match=r"\(2, 3, 35, 133\)"):
    sm(dev(d1), dev(g1[:, :1]))
  with pytest.raises(RuntimeError, match="contiguous fp32"):
    sm(dev(d1).double(), dev(g1))
  with pytest.raises(RuntimeError, match="uint8"):
    sm(dev(d1), dev(g1), dev(d1))
  with pytest.raises(RuntimeError, match="nothing has been smoothed"):
    smooth.DisparitySmoother(H, W, batch=B, device=DEV).fractions()


def test_three_iterations_equal_three_applications(cases):
  shape = ds.ONE_TILE_PLUS
  B, H, W = shape
  case = cases[(shape, 3)]
  d, c, g = case["disp"], case["code_in"], case["guide"]
  sm = smooth.DisparitySmoother(H, W, batch=B, radius=1, sigma_color=0.2, fill=True, min_support=3, iterations=3, device=DEV)
  want = ds.iterate(d, c, g, sm.weight_table(), 3, radius=1, fill=True, min_support=3)
  once = ds.wmedian(d, c, g, sm.weight_table(), 1, True, 3)
  assert want["counts"][0, 3] < once["counts"][0, 3], "the fill grows into the hole pass by pass"
  src = dev(d)
  r = sm(src, dev(g), dev(c))
  assert_same(dict(out=r.disp, code=r.code, counts=r.counts), want)
  assert same_bits(src, d)
  two = smooth.DisparitySmoother(H, W, batch=B, radius=1, fill=True, min_support=3, iterations=2, device=DEV)
  r = two(dev(d), code_in=dev(c))
  assert_same(dict(out=r.disp, code=r.code, counts=r.counts), ds.iterate(d, c, None, None, 2, radius=1, fill=True, min_support=3))


def test_captured_smoother_replayed_on_fresh_inputs_equals_eager(cases):
  shape = ds.TWO_TILES_PLUS
  B, H, W = shape
  case = cases[(shape, 3)]
  d1, c1, g1, _ = ds.random_case(shape, seed=9)
  sm = smooth.DisparitySmoother(H, W, batch=B, radius=3, sigma_color=0.1, fill=True, iterations=2, device=DEV)
  eager = [t.clone() for t in sm(dev(d1), dev(g1), dev(c1))]
  static = [dev(case["disp"]), dev(case["guide"]), dev(case["code_in"])]
  run = lambda: sm(*static)
  graph, result = capture.warm_up_and_capture(run, 1, run)
  for turn in range(2):                                              # and again: the counts are cleared inside the graph
    for t, a in zip(static, (d1, g1, c1)):
      t.copy_(dev(a))
    graph.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(result._fields, result, eager):
      assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "%s differs between replay %d and eager" % (name, turn)
  want = ds.iterate(d1, c1, g1, sm.weight_table(), 2, radius=3, fill=True, min_support=25)
  assert_same(dict(out=result.disp, code=result.code, counts=result.counts), want)


def test_refusals_set_the_error_and_launch_nothing():
  import re
  lib = nat.load()
  B, H, W = 1, 2, 8
  x = torch.zeros(B, 1, H, W, device=DEV)
  gd = torch.zeros(B, 3, H, W, device=DEV)
  lut = torch.ones(ds.LUT_SIZE, dtype=torch.int32, device=DEV)
  out, code = Guarded(B * H * W, torch.float32, SENTINEL), Guarded(B * H * W, torch.uint8, SENTINEL_U8)
  counts = Guarded(B * ds.COUNTS, torch.int32, SENTINEL_I32)
  px, pg, pl, po, pc, pn, s = nat.ptr(x), nat.ptr(gd), nat.ptr(lut), nat.ptr(out.view), nat.ptr(code.view), nat.ptr(counts.view), nat.stream()
  refused = [((None, None, None, 0, None, B, H, W, 1, 0, 1, po, pc, pn, s), "null"),
             ((px, None, None, 0, None, B, H, W, 1, 0, 1, None, pc, pn, s), "null"),
             ((px, None, None, 0, None, B, 0, W, 1, 0, 1, po, pc, pn, s), "shape"),
             ((px, None, pg, 2, pl, B, H, W, 1, 0, 1, po, pc, pn, s), "C 2"),
             ((px, None, pg, 3, None, B, H, W, 1, 0, 1, po, pc, pn, s), "guide"),
             ((px, None, None, 0, pl, B, H, W, 1, 0, 1, po, pc, pn, s), "guide"),
             ((px, None, None, 0, None, B, H, W, 8, 0, 1, po, pc, pn, s), "radius"),
             ((px, None, None, 0, None, B, H, W, 1, 2, 1, po, pc, pn, s), "fill"),
             ((px, None, None, 0, None, B, H, W, 1, 1, 0, po, pc, pn, s), "min_support"),
             ((px, None, None, 0, None, B, H, W, 1, 0, 1, px, pc, pn, s), "alias"),
             ((px, None, pg, 3, pl, B, H, W, 1, 0, 1, pg, pc, pn, s), "alias"),
             ((px, None, None, 0, None, B, H, W, 1, 0, 1, po, pc, po, s), "alias")]
  for args, word in refused:
    assert lib.as_disp_wmedian(*args) == -1, word
    assert re.search(word, lib.as_last_error().decode()), (word, lib.as_last_error())
  torch.cuda.synchronize()
  assert out.untouched() and code.untouched() and counts.untouched() and not bool(x.any()) and not bool(gd.any())


# ================================================================================================= where it plugs in
B, H, W, K, MAXDISP = 2, 83, 150, 3, 100
MODEL_FILTER = dict(edge_tol_abs=0.5, edge_tol_rel=0.0, max_diff=0.25, max_size=30)


@pytest.fixture(scope="module")
def world():
  """the networks in eval mode and a batch of pairs on the device (as tests/test_gpu_disp_filter.py builds them)"""
  fnet, snet = build(dict(k=K, s=0, maxdisp=MAXDISP, gain=200.0))
  fnet.eval(); snet.eval()
  left, right = syn.stereo_pair(B, H, W, seed=7, disparities=(3.0, 9.0, 14.0)[:B])
  return dict(fnet=fnet, snet=snet, pair=(left.to(DEV).contiguous(), right.to(DEV).contiguous()))


def _native_calls(monkeypatch, run):
  """the names of the entry points `run()` reaches through _native.call, in order, and run()'s result"""
  names, real = [], nat.call

  def recording(name, *args):
    names.append(name)
    return real(name, *args)
  monkeypatch.setattr(nat, "call", recording)
  try:
    result = run()
  finally:
    monkeypatch.setattr(nat, "call", real)
  return names, result


def test_filtered_both_view_inference_with_and_without_smoothing(world, monkeypatch):
  fnet, snet = world["fnet"], world["snet"]
  left, right = world["pair"]
  off = dfm.FilteredBothViewInference(fnet, snet, H, W, batch=B, **MODEL_FILTER)
  assert off.smoother is None
  off(left, right)                                                   # the first call records the plan; the second runs it
  calls_off, r_off = _native_calls(monkeypatch, lambda: off(left, right))
  torch.cuda.synchronize()
  assert len(r_off) == 5 and "as_disp_wmedian" not in calls_off
  assert [c for c in calls_off if c.startswith(("as_lr_", "as_disp_"))] == ["as_lr_check", "as_disp_edge_check", "as_disp_speckle", "as_lr_fill"]
  kept = [t.clone() for t in (r_off[0], r_off[1]) + tuple(r_off[2]) + tuple(r_off[3]) + (r_off[4],)]

  on = dfm.FilteredBothViewInference(fnet, snet, H, W, batch=B, smooth_radius=2, smooth_sigma=0.1, smooth_fill=True, **MODEL_FILTER)
  on(left, right)
  calls_on, r_on = _native_calls(monkeypatch, lambda: on(left, right))
  torch.cuda.synchronize()
  assert calls_on == calls_off + ["as_disp_wmedian"], "the smoother is one call more, at the end"
  assert len(r_on) == 6 and isinstance(r_on[5], smooth.Smoothed)
  first_five = [r_on[0], r_on[1]] + list(r_on[2]) + list(r_on[3]) + [r_on[4]]
  for i, (a, b) in enumerate(zip(first_five, kept)):
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "output %d changes when smoothing is on" % i
  disp_l, filt = r_on[0].cpu().numpy(), r_on[3]
  want = ds.wmedian(disp_l, filt.code.cpu().numpy(), left.cpu().numpy(), ds.weight_table(0.1, 3), 2, True, 13)
  assert_same(dict(out=r_on[5].disp, code=r_on[5].code, counts=r_on[5].counts), want)
  print("smoothed left view: unchanged, changed, filled, rejected:", want["counts"].tolist())
  assert (want["counts"][:, 1] > 0).all() and (want["counts"][:, 2] > 0).all(), "the scene exercises the smoother"
  by_hand = smooth.DisparitySmoother(H, W, batch=B, radius=2, sigma_color=0.1, fill=True, device=DEV)(r_on[0], left, filt.code)
  for a, b in zip(by_hand, r_on[5]):
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
  eager = [t.clone() for t in r_on[5]]
  on.capture(left, right)
  replayed = on(left, right)
  torch.cuda.synchronize()
  assert len(replayed) == 6
  for a, b in zip(replayed[5], eager):
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "the smoother's output differs between replay and eager"
  plain = dfm.FilteredBothViewInference(fnet, snet, H, W, batch=B, smooth_radius=1, **MODEL_FILTER)
  sm = plain(left, right)[5]
  assert_same(dict(out=sm.disp, code=sm.code, counts=sm.counts), ds.wmedian(disp_l, filt.code.cpu().numpy(), None, None, 1, False, 5))


def test_proxy_labeler_with_the_median_equals_the_stages_chained_by_hand(monkeypatch):
  from test_gpu_sgm import PB, PD, PH, PROXY, PW, proxy_pairs
  (l0, r0), (l1, r1) = proxy_pairs()
  off = sgm_mod.ProxyLabeler(PH, PW, batch=PB, maxdisp=PD, device=DEV, **PROXY)
  assert off.medians is None and off.median_radius == 0
  calls_off, _ = _native_calls(monkeypatch, lambda: off(dev(l1), dev(r1)))
  assert calls_off == ["as_sgm_census", "as_sgm_census", "as_sgm_aggregate", "as_sgm_select", "as_lr_check", "as_disp_speckle"]
  raw = {k: getattr(off.matcher.result(), k).cpu().numpy() for k in ("disp_l", "disp_r", "code_l", "code_r")}
  lab = sgm_mod.ProxyLabeler(PH, PW, batch=PB, maxdisp=PD, median_radius=1, device=DEV, **PROXY)
  calls_on, (labels, code, counts) = _native_calls(monkeypatch, lambda: lab(dev(l1), dev(r1)))
  torch.cuda.synchronize()
  assert calls_on == calls_off[:4] + ["as_disp_wmedian", "as_disp_wmedian"] + calls_off[4:]
  med_l = ds.wmedian(raw["disp_l"], raw["code_l"], None, None, 1, False, 5)
  med_r = ds.wmedian(raw["disp_r"], raw["code_r"], None, None, 1, False, 5)
  assert med_l["counts"][:, 1].min() > 0 and np.isnan(med_l["out"]).any()
  chk = lr.lr_check(med_l["out"], med_r["out"], PROXY["tol_abs"], 0.0)
  spk = df.speckle(med_l["out"], chk["code_l"], PROXY["max_diff"], PROXY["max_size"])
  want_labels = np.where(spk["code"] == 0, med_l["out"], F(0.0)).astype(F)
  assert same_bits(labels, want_labels) and same_bits(code, spk["code"]) and same_bits(counts, spk["counts"])
  disp_l, chain_code, _ = lab.chain(dev(l1), dev(r1))                # what OnlineAdapter(proxy_labeler=...) reads: the smoothed map
  assert same_bits(disp_l, med_l["out"]) and same_bits(chain_code, spk["code"])
  eager = [t.clone() for t in (labels, code, counts)]
  lab.capture(dev(l0), dev(r0))
  for a, b in zip(lab(dev(l1), dev(r1)), eager):
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "replay differs from eager"


def test_evaluate_model_and_sgm_baseline_report_the_smoothed_figures(tmp_path, capsys):
  import evaluate_model as E
  import sgm_baseline as SB
  from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
  k, h, w, n = 3, 64, 96, 3
  data, splits = make_tree(str(tmp_path), "KittiStereo2015", n=n, H0=70, W0=110, seed=3)
  weights = str(tmp_path / "weights")
  os.makedirs(weights)
  fnet, snet = FeatureExtractorNetwork(k), StereoNet(k, 1, 0)
  torch.save(syn.synthetic_state_dict(fnet.state_dict(), seed=123), os.path.join(weights, "feature_net.pth"))
  torch.save(syn.synthetic_state_dict(snet.state_dict(), seed=123, logit_gain=5.0), os.path.join(weights, "stereo_net.pth"))
  common = ["--dataset_path", data, "--dataset_name", "KittiStereo2015", "--split", "tiny", "--subsplit", "train",
            "--splits_path", splits, "--batch_size", "2", "--height", str(h), "--width", str(w), "--num_workers", "0"]
  args = ["--mode", "eval", "--load_weights_folder", weights, "--stereonet_k", str(k)] + common
  capsys.readouterr()
  E.main(E.make_parser().parse_args(args))
  assert "median" not in capsys.readouterr().out                     # default off
  E.main(E.make_parser().parse_args(args + ["--smooth_radius", "1"]))
  out = capsys.readouterr().out
  assert "before the plain median of radius 1:" in out and "after the plain median of radius 1:" in out
  import ast
  plain = ast.literal_eval(out.split("after the plain median of radius 1:")[1].splitlines()[0].strip())
  assert plain["density"] == 1.0, "every pixel of the network's map is usable and stays so"
  flags = ["--lr_check", "--post_filter", "--edge_tol", "0.5", "--smooth_radius", "2", "--smooth_sigma", "0.1", "--smooth_fill"]
  E.main(E.make_parser().parse_args(args + flags))
  out = capsys.readouterr().out
  assert "after the weighted median (sigma 0.1) of radius 2, filling:" in out
  before = ast.literal_eval(out.split("before the weighted median (sigma 0.1) of radius 2:")[1].splitlines()[0].strip())
  after = ast.literal_eval(out.split("of radius 2, filling:")[1].splitlines()[0].strip())
  assert set(before) == set(after) == {"EPE", "D1_all_2px", "D1_all_3px", "D1_all_4px", "D1_all_5px", "density"}
  assert 0.0 <= before["density"] <= after["density"] <= 1.0, "the fill only adds pixels"
  got = SB.main(SB.make_parser().parse_args(common + ["--maxdisp", "32", "--median", "1", "--proxy"]))
  assert set(got) == {"sgm", "sgm_median", "proxy"} and "3 x 3 median" in capsys.readouterr().out
  assert 0.0 < got["sgm_median"]["density"] == got["sgm"]["density"], "the plain median without fill keeps the same pixels"
  assert set(SB.main(SB.make_parser().parse_args(common + ["--maxdisp", "32"]))) == {"sgm"}
