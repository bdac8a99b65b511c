"""csrc/ood.hip (as_fcs_scores) and adaptive_stereo/ood.py on the GPU.

References, none of them the kernel under test: the reference's own max - torch.median maps (tests/golden/ood_fcs.npz), the
fcs output of as_softargmax_fwd for the mean map (bit for bit), tests/ood_ref.py (held to the fixture by
tests/test_ood_ref_cpu.py) for the fp64 per-image means and the precision/recall counts.

The bound on a score: every term of a map's sum is >= 0 or the sum is NaN, an fp64 accumulation of at most 2^24 fp32 terms is off
by far less than half an fp32 ulp, which leaves the final rounding: 1 ulp of fp32 against float32(fp64 mean of the reference map).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ood_ref as R
from adaptive_stereo import _native as nat
from adaptive_stereo import ood
from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
from adaptive_stereo.utils import synthetic as syn
from adaptive_stereo.utils.feature_contrast import feature_contrast_mean, feature_contrast_median
from conftest import GOLDEN_DIR, parity_note

DEV = "cuda:0"
SENTINEL = -7777.0
CASES = [(shape, gain) for shape in R.SHAPES for gain in R.GAINS]
IDS = [R.case_name(s, g) for s, g in CASES]


@pytest.fixture(scope="module")
def fixture():
  return np.load(os.path.join(GOLDEN_DIR, "ood_fcs.npz"), allow_pickle=False)


def run(vol, mean=True, median=True, scores=True, capacity=None, cursor=None, dropped=None):
  """as_fcs_scores on a numpy or device volume -> (fcs_mean, fcs_median, scores) device tensors, sentinel-filled where the
  output was not requested."""
  x = torch.from_numpy(vol).to(DEV) if isinstance(vol, np.ndarray) else vol
  B, D, H, W = x.shape
  capacity = B if capacity is None else capacity
  fm = torch.full((B, H, W), SENTINEL, device=DEV)
  fd = torch.full((B, H, W), SENTINEL, device=DEV)
  sc = torch.full((capacity, 2), SENTINEL, device=DEV)
  nat.call("as_fcs_scores", nat.ptr(x), B, D, H, W, nat.ptr(fm) if mean else None, nat.ptr(fd) if median else None,
           nat.ptr(sc) if scores else None, capacity if scores else 0, nat.ptr(cursor), nat.ptr(dropped), nat.stream())
  return fm, fd, sc


def softargmax_fcs(vol):
  """The fcs by-product of the existing soft-argmax kernel: the contract of the mean map."""
  x = torch.from_numpy(vol).to(DEV)
  B, D, H, W = x.shape
  pred = torch.empty(B, H, W, device=DEV)
  fcs = torch.empty(B, H, W, device=DEV)
  nat.call("as_softargmax_fwd", nat.ptr(x), B, D, H, W, nat.ptr(pred), None, nat.ptr(fcs), nat.stream())
  return fcs


def bits(t):
  return t.contiguous().view(torch.int32)


def assert_scores_within_1_ulp(got, want, what):
  gap = R.ulp_gap(got, want)
  print("%s: scores %s reference %s worst gap %s ulp" % (what, got.tolist(), want.tolist(), gap.max()))
  assert bool((gap <= 1.0).all()), "%s: %s ulp" % (what, gap.tolist())
  return float(gap.max())


@pytest.mark.parametrize("shape,gain", CASES, ids=IDS)
def test_maps_and_scores(fixture, shape, gain):
  name = R.case_name(shape, gain)
  # the fixture's volume, planted pixels and NaN included: the median map is the reference's, exactly
  vol = R.make_volume(shape, gain)
  assert np.array_equal(R.checksum(vol), fixture["check__" + name])
  fm, fd, sc = run(vol)
  want_median = fixture["median__" + name]
  got_median = fd.cpu().numpy()
  assert R.same_values(got_median, want_median), "median map != max - torch.median"
  assert R.same_values(got_median, R.fcs_median(vol))
  for kind, (b, p) in R.planted(shape).items():
    g, w = got_median.reshape(shape[0], -1)[b, p], want_median.reshape(shape[0], -1)[b, p]
    assert (np.isnan(g) and np.isnan(w)) if kind == "nan" else g == w, kind
  assert np.array_equal(np.isnan(fm.cpu().numpy()), R.has_nan(vol)), "a NaN among a pixel's values is a NaN in the mean map"
  gap_med = assert_scores_within_1_ulp(sc.cpu().numpy()[:, 1], R.image_scores(want_median, want_median)[:, 1], name + " median")

  # finite inputs (the same volume without its NaN): the mean map is as_softargmax_fwd's fcs, bit for bit
  vol = R.make_volume(shape, gain, nan=False)
  fm, fd, sc = run(vol)
  want_mean = softargmax_fcs(vol)
  assert torch.equal(bits(fm), bits(want_mean)), "mean map is not bit-identical to as_softargmax_fwd's fcs"
  if shape[1] <= 2:
    assert not bool(fm.any())
  want = R.image_scores(want_mean.cpu().numpy(), R.fcs_median(vol))
  gap = assert_scores_within_1_ulp(sc.cpu().numpy(), want, name)
  parity_note("ood_scores_" + name, worst_ulp=max(gap, gap_med))
  fm2, fd2, sc2 = run(vol)
  assert torch.equal(bits(sc), bits(sc2)) and torch.equal(bits(fm), bits(fm2)) and torch.equal(bits(fd), bits(fd2)), \
      "two runs on the same input differ"


def test_d_beyond_64_is_refused_before_any_launch():
  x = torch.zeros(1, 65, 2, 3, device=DEV)
  fm = torch.full((1, 2, 3), SENTINEL, device=DEV); fd = fm.clone(); sc = torch.full((1, 2), SENTINEL, device=DEV)
  state = torch.tensor([3, 5], dtype=torch.int32, device=DEV)
  lib = nat.load()
  rc = lib.as_fcs_scores(nat.ptr(x), 1, 65, 2, 3, nat.ptr(fm), nat.ptr(fd), nat.ptr(sc), 1, nat.ptr(state[0:1]),
                         nat.ptr(state[1:2]), nat.stream())
  assert rc != 0 and b"D 65" in lib.as_last_error()
  torch.cuda.synchronize()
  assert bool((fm == SENTINEL).all()) and bool((fd == SENTINEL).all()) and bool((sc == SENTINEL).all())
  assert state.tolist() == [3, 5]
  with pytest.raises(RuntimeError, match="D 65"):
    ood.fcs_scores(x)
  assert lib.as_fcs_scores(nat.ptr(x), 1, 0, 2, 3, nat.ptr(fm), None, None, 0, None, None, nat.stream()) != 0
  assert lib.as_fcs_scores(nat.ptr(x), 1, 12, 2, 3, None, None, None, 0, None, None, nat.stream()) != 0      # no output


def test_nan_poisons_its_pixel_and_its_image_only():
  shape = (3, 24, 7, 131)
  clean = R.make_volume(shape, 1.0, nan=False)
  fm0, fd0, sc0 = run(clean)
  dirty = clean.copy()
  dirty[1, 17, 3, 100] = np.float32("nan")
  fm, fd, sc = run(dirty)
  for a, a0 in ((fm, fm0), (fd, fd0)):
    assert bool(torch.isnan(a[1, 3, 100]))
    a = a.clone(); a[1, 3, 100] = a0[1, 3, 100]
    assert torch.equal(bits(a), bits(a0)), "another pixel changed"
  assert bool(torch.isnan(sc[1]).all())
  assert torch.equal(bits(sc[0]), bits(sc0[0])) and torch.equal(bits(sc[2]), bits(sc0[2]))


@pytest.mark.parametrize("mean,median,scores", [(True, True, False), (False, False, True), (True, False, False),
                                               (False, True, False), (True, False, True), (False, True, True)])
def test_null_outputs_leave_the_other_buffers_alone(mean, median, scores):
  vol = R.make_volume((2, 12, 5, 67), 1.0, nan=False)
  full = run(vol)
  part = run(vol, mean=mean, median=median, scores=scores)
  for asked, got, want in zip((mean, median, scores), part, full):
    if asked:
      assert torch.equal(bits(got), bits(want))
    else:
      assert bool((got == SENTINEL).all())


def test_rows_land_at_the_cursor_and_stop_at_capacity():
  """The C entry point itself: cursor 4 of capacity 6 and B = 3 -> rows 4 and 5 written, one dropped, cursor 7; without a
  cursor rows start at 0; a cursor past the capacity writes nothing."""
  vol = R.make_volume((3, 24, 7, 131), 1.0, nan=False)
  want = run(vol)[2]
  state = torch.tensor([4, 10], dtype=torch.int32, device=DEV)
  sc = run(vol, False, False, True, capacity=6, cursor=state[0:1], dropped=state[1:2])[2]
  assert state.tolist() == [7, 11]
  assert torch.equal(bits(sc[4:6]), bits(want[0:2])) and bool((sc[:4] == SENTINEL).all())
  sc = run(vol, False, False, True, capacity=6, cursor=state[0:1], dropped=state[1:2])[2]
  assert state.tolist() == [10, 14] and bool((sc == SENTINEL).all())
  sc = run(vol, False, False, True, capacity=2, dropped=state[1:2])[2]           # no cursor: rows 0, 1; the third is dropped
  assert state.tolist() == [10, 15] and torch.equal(bits(sc), bits(want[0:2]))


# ---- the collector ----------------------------------------------------------------------------------------------------------
def test_collector_appends_counts_drops_and_resets():
  vols = [torch.from_numpy(R.make_volume((b, 12, 5, 67), g, nan=False)).to(DEV) for b, g in ((2, 1.0), (3, 50.0), (2, 1.0))]
  vols[2] = vols[2] * 0.5
  want = torch.cat([ood.fcs_scores(v) for v in vols])
  col = ood.FcsCollector(6, device=DEV)
  for v in vols:
    col.add(v)
  got = col.scores()
  assert got.shape == (6, 2) and torch.equal(bits(got), bits(want[:6]))
  assert col.dropped() == 1
  col.reset()
  assert col.scores().shape == (0, 2) and col.dropped() == 0
  col.add(vols[1])
  assert torch.equal(bits(col.scores()), bits(want[2:5]))                        # row 0 is in use again
  torch.cuda.synchronize()
  before = torch.cuda.memory_allocated()
  col.add(vols[0])
  assert torch.cuda.memory_allocated() == before, "add() allocated"
  with pytest.raises(RuntimeError, match="no CPU path"):
    col.add(vols[0].cpu())
  with pytest.raises(RuntimeError, match="contiguous fp32"):
    col.add(vols[0].transpose(2, 3))


def test_collector_in_a_captured_graph_appends_on_every_replay():
  shape = (2, 12, 5, 67)
  contents = [R.make_volume(shape, 1.0, nan=False) * np.float32(s) for s in (1.0, 0.25, 3.0)]
  eager = [ood.fcs_scores(torch.from_numpy(c).to(DEV)) for c in contents]
  static = torch.from_numpy(contents[0]).to(DEV)
  col = ood.FcsCollector(8, device=DEV)
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    col.add(static)                                        # warm-up outside the capture
  torch.cuda.synchronize()
  col.reset()
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):     # one stream: a linear graph
    col.add(static)
  for c in contents:
    static.copy_(torch.from_numpy(c))
    graph.replay()
  torch.cuda.synchronize()
  got = col.scores()
  assert got.shape == (6, 2) and col.dropped() == 0
  assert torch.equal(bits(got), bits(torch.cat(eager)))


# ---- the module functions -----------------------------------------------------------------------------------------------------
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


def test_feature_contrast_median_on_the_models_logits(nets):
  fnet, snet = nets
  left, right = syn.stereo_pair(2, 96, 256, seed=1)
  cv = eager_cost_volume(fnet, snet, left.to(DEV), right.to(DEV))
  assert tuple(cv.shape) == (2, 12, 6, 16)
  got = feature_contrast_median(cv)
  want = cv.max(dim=1)[0] - cv.median(dim=1)[0]            # the reference's expression, on the device
  assert got.shape == want.shape and R.same_values(got.cpu().numpy(), want.cpu().numpy())
  assert R.same_values(got.cpu().numpy(), R.fcs_median(cv.cpu().numpy()))
  scores, fm, fd = ood.fcs_scores(cv, maps=True)
  assert torch.equal(bits(fd), bits(got)) and torch.equal(bits(fm), bits(softargmax_fcs(cv.cpu().numpy())))
  # the by-product StereoNet attaches comes from the fused tail kernel, which sums the D values as a tree: the same formula in
  # another order, so the bar of test_out_conv_softargmax_fcs at this gain (20), not bit equality
  by_product = feature_contrast_mean(cv)
  assert by_product is cv._as_fcs
  assert bool(((fm - by_product).abs() <= 1e-5 * 20.0 + 1e-5 * by_product.abs()).all())
  assert_scores_within_1_ulp(scores.cpu().numpy(), R.image_scores(fm.cpu().numpy(), fd.cpu().numpy()), "model logits")
  with pytest.raises(RuntimeError, match="no CPU path"):
    feature_contrast_median(cv.cpu())
  with pytest.raises(RuntimeError, match="no CPU path"):
    ood.fcs_scores(cv.cpu())


def test_collect_scores_over_synthetic_pairs(nets):
  fnet, snet = nets
  left, right = syn.stereo_pair(5, 96, 256, seed=3)
  batches = [{"color_l/0": left[i:i + 2], "color_r/0": right[i:i + 2]} for i in (0, 2, 4)]
  fnet.train(); snet.eval()
  try:
    got = ood.collect_scores(fnet, snet, batches, num_images=5)
    assert fnet.training and not snet.training, "the networks' training flags are not restored"
  finally:
    fnet.eval()
  assert got.shape == (5, 2) and got.is_cuda
  want32, want64 = [], []
  for b in batches:
    fcs = feature_contrast_mean(eager_cost_volume(fnet, snet, b["color_l/0"].to(DEV), b["color_r/0"].to(DEV)))
    want32.append(fcs.mean(dim=(-2, -1)))
    want64.append(fcs.double().mean(dim=(-2, -1)).float())
  assert bool((got > 0).all())
  # num_images below what the batches hold: the buffer is the bound, the surplus row is not returned
  assert torch.equal(bits(ood.collect_scores(fnet, snet, batches, num_images=3)), bits(got[:3]))
  assert_scores_within_1_ulp(got[:, 0].cpu().numpy(), torch.cat(want64).cpu().numpy(), "collect_scores vs fp64 mean")
  assert_scores_within_1_ulp(got[:, 0].cpu().numpy(), torch.cat(want32).cpu().numpy(), "collect_scores vs torch fp32 mean")


@pytest.mark.parametrize("n", [1, 7, 1000])
def test_precision_recall_on_the_device_is_the_double_loop(n):
  rs = np.random.RandomState(100 + n)
  novel = (10.0 + 2.0 * rs.standard_normal(n)).astype(np.float32)
  train = (13.0 + 1.5 * rs.standard_normal(n)).astype(np.float32)
  got = ood.precision_recall(torch.from_numpy(train).to(DEV), torch.from_numpy(novel).to(DEV), 100)
  want = R.precision_recall_loop(train, novel, 100)
  assert np.array_equal(got["cutoffs"], np.array(want["cutoffs"], np.float32))
  for k in ("tp", "fn", "tn", "fp"):
    assert got[k].tolist() == want[k], k
  assert got["precision"].tolist() == want["precision"] and got["recall"].tolist() == want["recall"]
