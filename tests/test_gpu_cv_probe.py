"""csrc/cv_probe.hip (as_cost_volume_probe), adaptive_stereo/cv_probe.py and cost_volume_analysis.py on the GPU.

References, none of them the kernel under test: tests/cv_probe_ref.py (held to the reference's own picks and values by
tests/test_cv_probe_ref_cpu.py), the mean map of as_fcs_scores and the fcs of as_softargmax_fwd (bit for bit at the picked
pixels), torch.argmax / torch.argmin on the device, numpy's sort in fp64 for the profile.

Bounds.  Picks, slices and the four values f, m1, m2, mean_rest are exact: the contract fixes every operation and its order.
A profile entry is an fp64 sum of at most 2^30 fp32 terms, off by far less than half an fp32 ulp, then one rounding: 1 ulp of fp32
against float32(fp64 mean), the bar of test_gpu_ood.py for the scores.  profile[0] - mean(profile[2:]) is, in exact arithmetic, the
mean over the pixels of max - mean(rest), which the per-image FCS score computes with one fp32 mean_rest per pixel: the two agree
within the mean over the pixels of cv_probe_ref.rounding_bound.
"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cv_probe_ref as R
import ood_ref
from adaptive_stereo import _native as nat
from adaptive_stereo import capture, cv_probe, ood
from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
from adaptive_stereo.utils import synthetic as syn
from conftest import parity_note

DEV = "cuda:0"
SENTINEL = -7777
OWN_NAMES = [c[0] for c in R.OWN_CASES]


def bits(t):
  return t.contiguous().view(torch.int32)


def run(vol, gt=None, pix=True, vals=True, slices=True, profile=True, capacity=None, cursor=None, dropped=None):
  """as_cost_volume_probe on a numpy or device volume -> (pix, vals, slices, profile) device tensors, sentinel-filled where the
  output was not requested or the row not written."""
  x = torch.from_numpy(vol).to(DEV) if isinstance(vol, np.ndarray) else vol
  g = torch.from_numpy(gt).to(DEV) if isinstance(gt, np.ndarray) else gt
  B, D, H, W = x.shape
  capacity = B if capacity is None else capacity
  out = (torch.full((capacity, 2, 3), SENTINEL, dtype=torch.int32, device=DEV),
         torch.full((capacity, 2, 5), float(SENTINEL), device=DEV),
         torch.full((capacity, 2, D), float(SENTINEL), device=DEV),
         torch.full((capacity, D), float(SENTINEL), device=DEV))
  asked = (pix, vals, slices, profile)
  nat.call("as_cost_volume_probe", nat.ptr(x), nat.ptr(g), B, D, H, W, *[nat.ptr(t) if a else None for t, a in zip(out, asked)],
           capacity, nat.ptr(cursor), nat.ptr(dropped), nat.stream())
  return out


def fcs_mean_map(vol):
  x = torch.from_numpy(vol).to(DEV)
  B, D, H, W = x.shape
  fm = torch.empty(B, H, W, device=DEV)
  sc = torch.empty(B, 2, device=DEV)
  nat.call("as_fcs_scores", nat.ptr(x), B, D, H, W, nat.ptr(fm), None, nat.ptr(sc), B, None, None, nat.stream())
  return fm.cpu().numpy(), sc.cpu().numpy()


def softargmax_fcs(vol):
  x = torch.from_numpy(vol).to(DEV)
  B, D, H, W = x.shape
  pred = torch.empty(B, H, W, device=DEV)
  fcs = torch.empty(B, H, W, device=DEV)
  nat.call("as_softargmax_fwd", nat.ptr(x), B, D, H, W, nat.ptr(pred), None, nat.ptr(fcs), nat.stream())
  return fcs.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(name):
  """One run per case, shared by the tests: (volume, gt, forced picks, the restatement's outputs, the kernel's as numpy)."""
  vol, gt, forced = R.make_case(name)
  got = [t.cpu().numpy() for t in run(vol, gt)]
  for a in got:
    a.setflags(write=False)
  return vol, gt, forced, R.probe(vol, gt), dict(pix=got[0], vals=got[1], slices=got[2], profile=got[3])


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_every_case_against_the_restatement(name):
  vol, gt, forced, want, got = case(name)
  B, D, H, W = vol.shape
  print("%s: picks %s" % (name, got["pix"].tolist()))
  assert np.array_equal(got["pix"], want["pix"]), "row, col, d_max"
  assert np.array_equal(R.bits(got["slices"]), R.bits(want["slices"])), "the slices are not the pixels' logits bit for bit"
  assert np.array_equal(R.bits(got["vals"]), R.bits(want["vals"])), "f, m1, m2, mean_rest, gt: %s vs %s" % (got["vals"], want["vals"])
  for (b, which), p in forced.items():
    assert got["pix"][b, which, 0] * W + got["pix"][b, which, 1] == p

  # f is the gate's own map at that pixel: as_fcs_scores' mean map, and as_softargmax_fwd's fcs where the column is finite
  fm, scores = fcs_mean_map(vol)
  soft = softargmax_fcs(np.nan_to_num(vol, nan=0.0))
  for b in range(B):
    for which in range(2):
      p = int(want["p"][b, which])
      f = got["vals"][b, which, 0]
      assert R.bits(f) == R.bits(fm[b].ravel()[p]), "f is not as_fcs_scores' mean map at the pixel"
      if not np.isnan(vol[b].reshape(D, -1)[:, p]).any():
        assert R.bits(f) == R.bits(soft[b].ravel()[p]), "f is not as_softargmax_fwd's fcs at the pixel"
        m1, mean_rest = got["vals"][b, which, 1], got["vals"][b, which, 3]
        if D > 2:
          assert R.bits(f) == R.bits(np.float32(m1 - mean_rest))

  # the profile: 1 ulp against float32(fp64 mean of the sorted columns); NaN images all NaN
  gap = ood_ref.ulp_gap(got["profile"], want["profile"])
  print("%s: profile worst gap %s ulp" % (name, gap.max()))
  assert bool((gap <= 1.0).all()), gap.tolist()
  again = [t.cpu().numpy() for t in run(vol, gt)]
  for a, key in zip(again, ("pix", "vals", "slices", "profile")):
    assert np.array_equal(a.view(np.uint32), got[key].view(np.uint32)), "two runs on the same input differ in " + key

  # the FCS score is a linear functional of the profile
  worst_share = 0.0
  if D > 2:
    for b in range(B):
      if np.isnan(vol[b]).any():
        assert np.isnan(scores[b, 0])
        continue
      prof = got["profile"][b].astype(np.float64)
      functional = prof[0] - prof[2:].mean()
      cols = vol[b].reshape(D, -1).T
      bound = sum(R.rounding_bound(c)[0] for c in cols) / len(cols)
      err = abs(functional - float(scores[b, 0]))
      print("%s image %d: profile[0] - mean(profile[2:]) %.9g, score %.9g, |diff| %.3e, bound %.3e" % (
          name, b, functional, scores[b, 0], err, bound))
      assert err <= bound
      worst_share = max(worst_share, err / bound)
  parity_note("cv_probe_" + name, profile_worst_ulp=float(gap.max()), functional_share_of_bound=worst_share)


@pytest.mark.parametrize("name", OWN_NAMES)
def test_planted_ties_select_the_smaller_pixel(name):
  """The maximum at the last pixel, the minimum in a wave's last lane, ties between a later pixel on a lower lane and an earlier
  one on a higher lane, ties on the same lane two trips apart (one of them between -0 and +0), an image smaller than a wave."""
  vol, gt, forced, want, got = case(name)
  W = vol.shape[3]
  assert forced
  for (b, which), p in forced.items():
    assert (int(got["pix"][b, which, 0]), int(got["pix"][b, which, 1])) == (p // W, p % W)
    tied = np.flatnonzero(R.fmap(vol)[b].ravel() == got["vals"][b, which, 0])
    assert tied[0] == p, "not the first of the pixels holding the extreme (%s)" % tied.tolist()


def test_nan_selects_its_first_pixel_and_poisons_its_image_only():
  shape = (3, 24, 7, 131)
  clean = ood_ref.make_volume(shape, 1.0, nan=False)
  gt = np.random.RandomState(3).uniform(0, 24, (3, 1, 7, 131)).astype(np.float32)
  out0 = run(clean, gt)
  dirty = clean.copy()
  dirty[1, 2, 5, 7] = np.float32("nan")          # p = 662
  dirty[1, 17, 3, 100] = np.float32("nan")       # p = 493: the first one
  pix, vals, slices, profile = run(dirty, gt)
  assert pix[1].tolist() == [[3, 100, -1], [3, 100, -1]]
  assert bool((bits(vals[1, :, :4]) == 0x7FC00000).all())
  assert torch.equal(bits(vals[1, :, 4]), bits(torch.from_numpy(gt[1, 0, 3, 100:101]).to(DEV).expand(2)))
  assert torch.equal(bits(slices[1, 0]), bits(torch.from_numpy(dirty[1, :, 3, 100]).to(DEV)))
  assert bool(torch.isnan(profile[1]).all())
  for got, want in zip((pix, vals, slices, profile), out0):
    for b in (0, 2):
      assert torch.equal(bits(got[b]), bits(want[b])), "another image changed"


@pytest.mark.parametrize("asked", [(True, False, False, False), (False, True, False, False), (False, False, True, False),
                                   (False, False, False, True), (True, True, True, False), (False, True, False, True)])
def test_null_outputs_leave_the_other_buffers_alone(asked):
  vol, gt, _, _, _ = case("b2_d12_h5_w67_g1")
  full = run(vol, gt)
  part = run(vol, gt, *asked)
  for a, got, want in zip(asked, part, full):
    if a:
      assert torch.equal(bits(got), bits(want))
    else:
      assert bool((got == SENTINEL).all())


def test_rows_land_at_the_cursor_and_stop_at_capacity():
  """cursor 4 of capacity 6 and B = 3 -> rows 4 and 5 written, one dropped, cursor 7; a cursor past the capacity writes nothing;
  without a cursor rows start at 0."""
  vol, gt, _, _, _ = case("b3_d24_h7_w131_g1")
  want = run(vol, gt)
  state = torch.tensor([4, 10], dtype=torch.int32, device=DEV)
  out = run(vol, gt, capacity=6, cursor=state[0:1], dropped=state[1:2])
  assert state.tolist() == [7, 11]
  for got, w in zip(out, want):
    assert torch.equal(bits(got[4:6]), bits(w[0:2])) and bool((got[:4] == SENTINEL).all())
  out = run(vol, gt, capacity=6, cursor=state[0:1], dropped=state[1:2])
  assert state.tolist() == [10, 14] and all(bool((got == SENTINEL).all()) for got in out)
  out = run(vol, gt, capacity=2, dropped=state[1:2])
  assert state.tolist() == [10, 15]
  for got, w in zip(out, want):
    assert torch.equal(bits(got), bits(w[0:2]))


def test_bad_arguments_touch_nothing():
  x = torch.zeros(1, 65, 2, 3, device=DEV)
  state = torch.tensor([3, 5], dtype=torch.int32, device=DEV)
  pix = torch.full((1, 2, 3), SENTINEL, dtype=torch.int32, device=DEV)
  lib = nat.load()
  rc = lib.as_cost_volume_probe(nat.ptr(x), None, 1, 65, 2, 3, nat.ptr(pix), None, None, None, 1, nat.ptr(state[0:1]),
                                nat.ptr(state[1:2]), nat.stream())
  assert rc != 0 and b"D 65" in lib.as_last_error()
  torch.cuda.synchronize()
  assert bool((pix == SENTINEL).all()) and state.tolist() == [3, 5]
  with pytest.raises(RuntimeError, match="D 65"):
    cv_probe.probe_cost_volume(x)


# ---- the Python layer --------------------------------------------------------------------------------------------------------
def test_probe_cost_volume_and_its_named_views():
  vol, gt, _, want, got = case("b4_d12_h24_w78_g1")
  res = cv_probe.probe_cost_volume(torch.from_numpy(vol).to(DEV), torch.from_numpy(gt).to(DEV), profile=True)
  assert len(res) == 4 and res.pix.shape == (4, 2, 3) and res.vals.shape == (4, 2, 5) and res.slices.shape == (4, 2, 12)
  assert res.profile.shape == (4, 12) and res.pix.dtype == torch.int32
  for key in ("pix", "vals", "slices", "profile"):
    assert np.array_equal(getattr(res, key).cpu().numpy().view(np.uint32), got[key].view(np.uint32))
  assert torch.equal(res.row, res.pix[..., 0]) and torch.equal(res.col, res.pix[..., 1]) and torch.equal(res.d_max, res.pix[..., 2])
  for i, view in enumerate((res.fcs, res.max, res.second, res.mean_rest, res.gt)):
    assert torch.equal(bits(view), bits(res.vals[..., i]))
  without = cv_probe.probe_cost_volume(torch.from_numpy(vol).to(DEV))
  assert without.profile is None and bool(torch.isnan(without.gt).all())
  assert torch.equal(bits(without.vals[..., :4]), bits(res.vals[..., :4]))
  with pytest.raises(RuntimeError, match="gt must be"):
    cv_probe.probe_cost_volume(torch.from_numpy(vol).to(DEV), torch.zeros(4, 1, 24, 77, device=DEV))


def test_collector_appends_counts_drops_and_resets():
  vols = [torch.from_numpy(ood_ref.make_volume((b, 12, 5, 67), g, nan=False)).to(DEV) for b, g in ((2, 1.0), (3, 50.0), (2, 1.0))]
  vols[2] = vols[2] * 0.5
  gts = [torch.rand(v.shape[0], 1, 5, 67, device=DEV) * 12 for v in vols]
  each = [cv_probe.probe_cost_volume(v, g, profile=True) for v, g in zip(vols, gts)]
  col = cv_probe.CostVolumeProbe(6, 12, profile=True, device=DEV)
  for v, g in zip(vols, gts):
    col.add(v, g)
  got = col.results()
  assert len(got) == 6 and col.dropped() == 1
  for key in ("pix", "vals", "slices", "profile"):
    assert torch.equal(bits(getattr(got, key)), bits(torch.cat([getattr(e, key) for e in each])[:6])), key
  col.reset()
  assert len(col.results()) == 0 and col.dropped() == 0
  col.add(vols[1], gts[1])
  assert torch.equal(bits(col.results().vals), bits(each[1].vals))          # row 0 is in use again
  torch.cuda.synchronize()
  before = torch.cuda.memory_allocated()
  col.add(vols[0])
  assert torch.cuda.memory_allocated() == before, "add() allocated"
  with pytest.raises(RuntimeError, match="no CPU path"):
    col.add(vols[0].cpu())
  with pytest.raises(RuntimeError, match="contiguous fp32"):
    col.add(vols[0].transpose(2, 3))
  with pytest.raises(RuntimeError, match="D 24"):
    col.add(torch.zeros(1, 24, 5, 67, device=DEV))


def test_collector_in_a_captured_graph_appends_on_every_replay():
  shape = (2, 12, 5, 67)
  contents = [ood_ref.make_volume(shape, 1.0, nan=False) * np.float32(s) for s in (1.0, 0.25, 3.0)]
  gt = torch.rand(2, 1, 5, 67, device=DEV) * 12
  eager = [cv_probe.probe_cost_volume(torch.from_numpy(c).to(DEV), gt, profile=True) for c in contents]
  static = torch.from_numpy(contents[0]).to(DEV)
  col = cv_probe.CostVolumeProbe(8, 12, profile=True, device=DEV)
  graph, _ = capture.warm_up_and_capture(lambda: col.add(static, gt), 1, lambda: col.add(static, gt),
                                         state=lambda: {"cursor_and_dropped": col._state})
  assert len(col.results()) == 0, "the warm-up left a row"
  for c in contents:
    static.copy_(torch.from_numpy(c))
    graph.replay()
  torch.cuda.synchronize()
  got = col.results()
  assert len(got) == 6 and col.dropped() == 0
  for key in ("pix", "vals", "slices", "profile"):
    assert torch.equal(bits(getattr(got, key)), bits(torch.cat([getattr(e, key) for e in eager]))), key


# ---- the model's own logits, collect_probes and the command line -----------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
  k = 4
  fnet, snet = FeatureExtractorNetwork(k), StereoNet(k, 1, 0, maxdisp=192)
  fnet.load_state_dict(syn.synthetic_state_dict(fnet.state_dict(), seed=123))
  snet.load_state_dict(syn.synthetic_state_dict(snet.state_dict(), seed=123, logit_gain=20.0))
  return fnet.to(DEV).eval(), snet.to(DEV).eval()


def eager_cost_volume(fnet, snet, left, right):
  with torch.no_grad():
    return snet(left, fnet(left), fnet(right), "l", output_cost_volume=True)["cost_volume_l/4"]


def test_picks_on_the_models_logits_are_torch_argmax_of_the_gates_map(nets):
  fnet, snet = nets
  left, right = syn.stereo_pair(2, 96, 256, seed=1)
  cv = eager_cost_volume(fnet, snet, left.to(DEV), right.to(DEV))
  assert tuple(cv.shape) == (2, 12, 6, 16)
  gt = torch.rand(2, 1, 6, 16, device=DEV, generator=torch.Generator(DEV).manual_seed(9)) * 12
  res = cv_probe.probe_cost_volume(cv, gt, profile=True)
  scores, fm, _ = ood.fcs_scores(cv, maps=True)
  flat = fm.flatten(1)
  want_p = torch.stack([torch.argmax(flat, dim=1), torch.argmin(flat, dim=1)], dim=1)
  assert torch.equal(res.row.long() * 16 + res.col.long(), want_p)
  for b in range(2):
    for which in range(2):
      r, c = int(res.row[b, which]), int(res.col[b, which])
      assert torch.equal(bits(res.slices[b, which]), bits(cv[b, :, r, c])), "the slice is not the gathered logits"
      assert torch.equal(bits(res.gt[b, which]), bits(gt[b, 0, r, c]))
      assert torch.equal(bits(res.fcs[b, which]), bits(fm[b, r, c]))
      assert int(res.d_max[b, which]) == int(torch.argmax(cv[b, :, r, c]))
  prof = res.profile.double()
  functional = prof[:, 0] - prof[:, 2:].mean(dim=1)
  cols = cv.cpu().numpy().reshape(2, 12, -1)
  for b in range(2):
    bound = sum(R.rounding_bound(c)[0] for c in cols[b].T) / cols.shape[2]
    assert abs(float(functional[b]) - float(scores[b, 0])) <= bound


def synthetic_samples(n, seed):
  left, right = syn.stereo_pair(n, 96, 256, seed=seed)
  gt = torch.rand(n, 1, 6, 16, generator=torch.Generator().manual_seed(seed)) * 12
  return [{"color_l/0": left[i], "color_r/0": right[i], "gt_disp_l/4": gt[i]} for i in range(n)]


def test_collect_probes_over_synthetic_pairs(nets):
  fnet, snet = nets
  samples = synthetic_samples(5, seed=3)
  batches = [{k: torch.stack([s[k] for s in samples[i:i + 2]]) for k in samples[0]} for i in (0, 2, 4)]
  seen = []
  fnet.train(); snet.eval()
  try:
    got = cv_probe.collect_probes(fnet, snet, batches, num_images=5, profile=True,
                                  on_batch=lambda first, cv, gt: seen.append((first, cv.clone(), gt.clone())))
    assert fnet.training and not snet.training, "the networks' training flags are not restored"
  finally:
    fnet.eval()
  assert len(got) == 5 and got.pix.is_cuda and got.profile.shape == (5, 12)
  assert [first for first, _, _ in seen] == [0, 2, 4]
  for (first, cv, gt), b in zip(seen, batches):
    # the rows are the probe of the very volume the pass produced; that volume is the eval-mode forward pass of the pair (the two
    # images go through the feature extractor as one batch there, apart here: a sanity bar, not a bit comparison)
    n = cv.shape[0]
    assert torch.equal(gt, b["gt_disp_l/4"].to(DEV))
    assert float((cv - eager_cost_volume(fnet, snet, b["color_l/0"].to(DEV), b["color_r/0"].to(DEV))).abs().max()) <= 1e-2
    want = cv_probe.probe_cost_volume(cv, gt, profile=True)
    for key in ("pix", "vals", "slices", "profile"):
      assert torch.equal(bits(getattr(got, key)[first:first + n]), bits(getattr(want, key))), key
  fewer = cv_probe.collect_probes(fnet, snet, batches, num_images=3)          # the buffer is the bound
  assert len(fewer) == 3 and fewer.profile is None and torch.equal(bits(fewer.vals), bits(got.vals[:3]))
  no_gt = cv_probe.collect_probes(fnet, snet, [{k: v for k, v in batches[0].items() if k != "gt_disp_l/4"}], num_images=2)
  assert bool(torch.isnan(no_gt.gt).all()) and torch.equal(no_gt.pix, got.pix[:2])


def test_command_line_save_and_curve_data(nets, tmp_path):
  import cost_volume_analysis as cva
  fnet, snet = nets
  samples = synthetic_samples(3, seed=5)
  folder = str(tmp_path / "train")
  probes = cva.save_probes(fnet, snet, samples, folder, num_images=2, save_volumes=True)
  stored = torch.load(os.path.join(folder, "probes.pt"))
  assert sorted(stored) == ["pix", "profile", "slices", "vals"] and stored["pix"].shape == (2, 2, 3)
  assert sorted(os.listdir(folder)) == ["0_cost_volume.pt", "0_gt.pt", "1_cost_volume.pt", "1_gt.pt", "probes.pt"]
  for i in range(2):
    cv = torch.load(os.path.join(folder, "%d_cost_volume.pt" % i))
    gt = torch.load(os.path.join(folder, "%d_gt.pt" % i))
    assert tuple(cv.shape) == (1, 12, 6, 16) and torch.equal(gt, samples[i]["gt_disp_l/4"].unsqueeze(0))
    want = cv_probe.probe_cost_volume(cv.to(DEV), gt.to(DEV), profile=True).cpu()
    for key in ("pix", "vals", "slices", "profile"):
      assert torch.equal(bits(stored[key][i:i + 1]), bits(getattr(want, key))), key
      assert torch.equal(bits(probes[key]), bits(stored[key]))
    for which, w in (("hi", 0), ("lo", 1)):
      c = cva.curve_data(stored, i, which)
      r, col = c["row"], c["col"]
      assert np.array_equal(c["curve"], cv[0, :, r, col].numpy()) and c["disparity"] == list(range(12))
      assert c["max"] == float(cv[0, :, r, col].max()) and c["gt"] == float(gt[0, 0, r, col])
      assert c["fcs"] == float(np.float32(c["max"]) - np.float32(c["mean_rest"])) and c["d_max"] == int(cv[0, :, r, col].argmax())


def test_command_line_visualize_writes_the_figures(nets, tmp_path):
  pytest.importorskip("matplotlib")
  import cost_volume_analysis as cva
  fnet, snet = nets
  for domain, seed in (("train", 5), ("novel", 6)):
    cva.save_probes(fnet, snet, synthetic_samples(2, seed=seed), str(tmp_path / domain), num_images=2)
  written = cva.visualize(str(tmp_path), num_images=2)
  names = sorted(os.path.relpath(p, str(tmp_path)) for p in written)
  assert names == ["novel/0_cost_volume_slice.pdf", "novel/1_cost_volume_slice.pdf", "rank_profile.pdf",
                   "train/0_cost_volume_slice.pdf", "train/1_cost_volume_slice.pdf"]
  for p in written:
    with open(p, "rb") as f:
      assert f.read(5) == b"%PDF-"


@pytest.mark.parametrize("D", [3, 5, 13, 25, 64])
@pytest.mark.parametrize("lead", [(2, 3, 70), (1, 9, 67)], ids=["210px_idle_lanes", "603px_second_pixel"])
def test_the_three_fcs_maps_are_one_map(lead, D):
  """csrc/column_stats.h is the one definition of the FCS loop: as_softargmax_fwd's fcs, as_fcs_scores' mean map and the fcs
  as_cost_volume_probe reports at its two picks are equal as int32 bit patterns, on a designed volume (ood_ref.make_volume:
  the maximum twice, all equal, signed zeros) at 210 pixels (lanes of the 512-lane workgroup idle) and at 603 (some lanes take a
  second pixel), for the first D of the 24- and 64-wide instances, the widest D and two narrow ones."""
  B, H, W = lead
  vol = ood_ref.make_volume((B, D, H, W), 20.0, nan=False)
  assert not np.isnan(vol).any()
  soft = softargmax_fcs(vol)
  fm, _ = fcs_mean_map(vol)
  assert np.array_equal(R.bits(soft), R.bits(fm)), "as_softargmax_fwd's fcs and as_fcs_scores' mean map differ"
  pix, vals, _, _ = [t.cpu().numpy() for t in run(vol, profile=False)]
  for b in range(B):
    for which, arg in ((cv_probe.HI, np.argmax), (cv_probe.LO, np.argmin)):
      row, col = int(pix[b, which, 0]), int(pix[b, which, 1])
      assert row * W + col == int(arg(fm[b].ravel())), "the pick is not the extreme of the map"
      f = vals[b, which, 0]
      assert R.bits(f) == R.bits(fm[b, row, col]) == R.bits(soft[b, row, col]), (b, which, f, fm[b, row, col], soft[b, row, col])
