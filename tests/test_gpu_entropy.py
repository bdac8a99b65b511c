"""csrc/entropy.hip (as_image_entropy) and adaptive_stereo/utils/entropy.py on the GPU.

References, none of them the kernel under test: the reference's own utils/entropy.py through tests/golden/entropy.npz, and
tests/entropy_ref.py (held to that fixture by tests/test_entropy_ref_cpu.py) for the counts and the fp64 entropies.

The bounds.  The counts are integers: `hist` must equal entropy_ref's counts bit for bit in every case.  A score is a sum of at
most 256 fp64 terms p * log2(p) of one sign, each good to a few fp64 ulps, so the sum is off by far less than half an fp32 ulp,
which leaves the final rounding: 1 ulp of fp32 against float32(entropy_ref's fp64 value).  Against the REFERENCE's fp32 results
the bound is that plus the reference's own measured distance from the fp64 value (tests/golden/entropy_bound.json, taken twice
as tests/test_entropy_ref_cpu.py takes it).

Every image sits in a buffer filled with 0.5 (a pixel that would be counted if it were read), scores and hist between sentinel
rows.
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import entropy_ref as R
from adaptive_stereo import _native as nat
from adaptive_stereo import ood
from adaptive_stereo.utils import entropy as E
from conftest import GOLDEN_DIR, parity_note

DEV = "cuda:0"
SENTINEL = -7777.0
HSENT = -77
GUARD = 16
BOUND = json.load(open(os.path.join(GOLDEN_DIR, "entropy_bound.json")))


@pytest.fixture(scope="module")
def fixture():
  return np.load(os.path.join(GOLDEN_DIR, "entropy.npz"), allow_pickle=False)


def bits(t):
  return t.contiguous().view(torch.int32)


def workspace(B):
  return torch.zeros(int(nat.load().as_image_entropy_workspace(B)), dtype=torch.uint8, device=DEV)


def run(images, offset=0, capacity=None, cursor=None, dropped=None, ws=None, want_hist=True):
  """as_image_entropy on numpy images [B,C,H,W] placed `offset` floats into a guarded buffer -> (scores [capacity,2],
  hist [B,2,256], workspace), after checking that the guards and sentinels around every buffer are untouched."""
  images = np.ascontiguousarray(images, np.float32)
  B, C, H, W = images.shape
  capacity = B if capacity is None else capacity
  buf = torch.full((GUARD + offset + images.size + GUARD,), 0.5, device=DEV)
  buf[GUARD + offset:GUARD + offset + images.size] = torch.from_numpy(images.reshape(-1)).to(DEV)
  x = buf[GUARD + offset:]
  sc = torch.full((capacity + 2, 2), SENTINEL, device=DEV)
  hist = torch.full((B + 2, 2, 256), HSENT, dtype=torch.int32, device=DEV)
  ws = workspace(B) if ws is None else ws
  nat.call("as_image_entropy", nat.ptr(x), B, C, H, W, nat.ptr(sc[1:]), capacity, nat.ptr(cursor), nat.ptr(dropped),
           nat.ptr(hist[1:]) if want_hist else None, nat.ptr(ws), nat.stream())
  torch.cuda.synchronize()
  assert bool((sc[0] == SENTINEL).all()) and bool((sc[-1] == SENTINEL).all()), "a score row outside [0, capacity) was written"
  assert bool((hist[0] == HSENT).all()) and bool((hist[-1] == HSENT).all()), "hist written outside [B][2][256]"
  assert not bool(ws.any()), "the workspace is not all zero after the call"
  return sc[1:-1], hist[1:-1], ws


def check(images, what, **kw):
  """hist bit for bit, scores within 1 ulp of float32(fp64); returns (scores, hist) as numpy."""
  images = np.ascontiguousarray(images, np.float32)
  want_sc, want_hist = R.batch(images)
  sc, hist, _ = run(images, **kw)
  got_hist = hist.cpu().numpy().astype(np.int64)
  assert np.array_equal(got_hist, want_hist.astype(np.int64)), "%s: counts differ at %s" % (
      what, np.argwhere(got_hist != want_hist.astype(np.int64))[:8].tolist())
  got_sc = sc.cpu().numpy()
  gap = R.ulp_gap(got_sc, want_sc)
  print("%s: scores %s reference %s worst gap %s ulp" % (what, got_sc.tolist(), want_sc.tolist(), gap.max()))
  assert bool((gap <= 1.0).all()), "%s: %s ulp" % (what, gap.tolist())
  return got_sc, got_hist


def rand_images(shape, seed, lo=0.0, hi=1.0):
  return (np.random.RandomState(seed).random_sample(shape) * (hi - lo) + lo).astype(np.float32)


# ---- the reference's own results -----------------------------------------------------------------------------------------------
def test_fixture_images_through_every_entry_point(fixture):
  worst = {"gray": 0.0, "grad": 0.0}
  for name in (str(n) for n in fixture["names"]):
    img = fixture["img__" + name]
    t = torch.from_numpy(img).to(DEV)
    planes = img.reshape((1, -1) + img.shape[-2:])
    got_sc, _ = check(planes, name)
    batched = E.image_entropy(t.reshape(planes.shape))
    assert torch.equal(bits(batched), bits(torch.from_numpy(got_sc).to(DEV)))
    named = {"gray": E.grayscale_shannon_entropy(t)}
    if img.ndim == 2:
      named["grad"] = E.gradient_shannon_entropy(t)
    for col, (key, h) in enumerate((k, named.get(k)) for k in ("gray", "grad")):
      if h is None:
        continue
      assert h.dim() == 0 and h.is_cuda and h.dtype == torch.float32
      assert torch.equal(bits(h.reshape(1)), bits(batched[0, col].reshape(1)))
      ref = fixture[key + "__" + name]
      if name in R.EXACT_BITS:
        assert float(h) == float(ref) == R.EXACT_BITS[name], name
      else:
        gap = float(R.ulp_gap(np.float32(float(h)), ref))
        assert gap <= 1.0 + 2.0 * BOUND["worst_ulp"][key], (name, key, gap)
        worst[key] = max(worst[key], gap)
  parity_note("entropy_vs_reference_fp32", worst_ulp_gray=worst["gray"], worst_ulp_grad=worst["grad"])
  with pytest.raises(AssertionError):
    E.gradient_shannon_entropy(torch.zeros(1, 4, 5, device=DEV))          # the reference's 2-D assertion
  with pytest.raises(RuntimeError, match="no CPU path"):
    E.grayscale_shannon_entropy(torch.zeros(1, 4, 5))
  with pytest.raises(RuntimeError, match="no CPU path"):
    E.image_entropy(torch.zeros(1, 1, 4, 5))


# ---- shape edges ---------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1, 1), (1, 1, 1, 7), (1, 1, 5, 1), (2, 3, 4, 1)] + [(1, 1, 3, w) for w in (2, 3, 5, 63, 64, 65, 257)] + \
         [(2, 2, 5, 257), (3, 3, 7, 65)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(str(s) for s in sh) for sh in SHAPES])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_shape_edges_and_unaligned_base(shape, offset):
  """offset: the base pointer that many floats past a 16-byte boundary, so the head, the tail and (W not a multiple of 4) every
  row's own alignment are exercised.  Values in [-0.1, 1.2]: some have no bin."""
  images = rand_images(shape, 7 + shape[3], -0.1, 1.2)
  sc, hist = check(images, "shape %s offset %d" % (shape, offset), offset=offset)
  if shape[3] == 1:
    assert np.isnan(sc[:, 1]).all() and not hist[:, 1].any() and not np.isnan(sc[:, 0]).any()


def test_images_and_planes_do_not_leak_into_each_other():
  B, C, H, W = 3, 3, 7, 65
  images = rand_images((B, C, H, W), 11)
  images[1] = images[1] * 0.25                     # three distinct distributions
  images[2] = 0.75
  sc, hist = check(images, "B=3 C=3")
  for b in range(B):
    alone_sc, alone_hist = check(images[b:b + 1], "image %d alone" % b)
    assert np.array_equal(alone_hist[0], hist[b]) and np.array_equal(alone_sc[0].view(np.int32), sc[b].view(np.int32))
  assert (hist[:, 0].sum(axis=1) == C * H * W).all() and (hist[:, 1].sum(axis=1) == C * H * (W - 1)).all()
  assert hist[2, 0, 191] == C * H * W and hist[2, 1, 128] == C * H * (W - 1)


@pytest.mark.parametrize("W", [5, 64, 65, 257])
def test_differences_stop_at_row_ends(W):
  """Constant rows alternating between 0 and 1: every difference inside a row is 0; one taken across a row end would be +-255."""
  H = 8
  images = np.zeros((2, 2, H, W), np.float32)
  images[:, :, 1::2] = 1.0
  images[1] = 1.0 - images[1]                      # the second image starts with a row of ones
  _, hist = check(images, "row ends W=%d" % W)
  want = np.zeros(256, np.int64); want[R.grad_bin(0)] = 2 * H * (W - 1)
  assert np.array_equal(hist[0, 1], want) and np.array_equal(hist[1, 1], want)
  assert hist[0, 0, 0] == hist[0, 0, 255] == H * W


# ---- contention and merging ----------------------------------------------------------------------------------------------------
def test_constant_kitti_image_puts_every_pixel_into_one_bin():
  H, W = 375, 1242
  images = np.full((1, 1, H, W), 0.4, np.float32)
  sc, hist = check(images, "constant 375x1242")
  assert hist[0, 0, 102] == 465750 and hist[0, 0].sum() == 465750          # more than 2^16 increments of one counter
  assert hist[0, 1, 128] == H * (W - 1) and hist[0, 1].sum() == H * (W - 1)
  assert sc[0, 0] == 0.0 and sc[0, 1] == 0.0


def test_several_workgroups_merge_into_one_image():
  images = rand_images((2, 1, 96, 256), 5)
  sc, hist = check(images, "random 96x256")
  assert (hist[:, 0, :255] > 0).all() and not hist[:, 0, 255].any(), "x in [0, 1) fills bins 0..254 at this size, never 255"
  sc2, hist2 = check(images, "random 96x256 again")
  assert np.array_equal(sc.view(np.int32), sc2.view(np.int32)) and np.array_equal(hist, hist2), "two runs differ"


# ---- rounding and range edges --------------------------------------------------------------------------------------------------
def test_rounding_range_edges_and_invalid_pixels():
  f = np.float32
  up, down = (lambda x: np.nextafter(f(x), f(np.inf))), (lambda x: np.nextafter(f(x), f(-np.inf)))
  row = []
  for k in (1, 3, 85, 127, 128, 254, 255):
    x = f(k) / f(255.0)
    row += [down(x), x, up(x)]
  row += [f(1.0), up(1.0), f(256) / f(255), f(-0.001), f(-1) / f(255), down(f(-1) / f(255)), f(0.0), f(-0.0)]
  images = np.array(row, np.float32).reshape(1, 1, 1, -1)
  _, hist = check(images, "k/255 neighbours and range edges")
  v, ok = R.quantise(images.reshape(-1))
  assert ok.all() and hist[0, 0].sum() == int(((v >= 0) & (v <= 255)).sum())
  single = lambda x: check(np.array([[[[x]]]], np.float32), "single %r" % float(x))[1][0, 0]
  assert single(f(1.0))[255] == 1 and single(up(1.0))[255] == 1, "x just above 1 still gives v = 255"
  assert single(f(256) / f(255)).sum() == 0 and single(f(-1) / f(255)).sum() == 0
  assert single(f(-0.001))[0] == 1, "-0.001 truncates toward zero into bin 0"

  pair = np.array([[[[300 / 255.0 + 1e-4, 100 / 255.0 + 1e-4]]]], np.float32)
  _, hist = check(pair, "(300, 100)")
  assert hist[0, 0].sum() == 1 and hist[0, 0, 100] == 1 and hist[0, 1, R.grad_bin(-200)] == 1 and hist[0, 1].sum() == 1

  # an invalid pixel enters no bin and spoils the two differences it takes part in; its neighbours' other differences count
  bad = [f("nan"), f("inf"), f("-inf"), f(1e10), f(-1e10), f(8421505.0)]
  W = 9
  images = np.full((len(bad) + 1, 1, 2, W), 0.5, np.float32)
  for b, x in enumerate(bad):
    images[b, 0, 0, 4] = x
    images[b, 0, 1, 0] = x                          # at a row start: one difference only
  images[len(bad), 0, 0, 4] = f(8421504.0)         # 255 x = 2147483520, the largest valid product: counted nowhere, spoils nothing else
  _, hist = check(images, "invalid pixels")
  for b in range(len(bad) + 1):
    lost_pixels = 2 if b < len(bad) else 1
    lost_pairs = 3 if b < len(bad) else 2
    assert hist[b, 0].sum() == 2 * W - lost_pixels and hist[b, 0, 127] == 2 * W - lost_pixels
    assert hist[b, 1].sum() == 2 * (W - 1) - lost_pairs and hist[b, 1, 128] == 2 * (W - 1) - lost_pairs


# ---- cursor, capacity, workspace, errors -----------------------------------------------------------------------------------------
def test_rows_land_at_the_cursor_and_the_workspace_cleans_itself():
  images = rand_images((3, 1, 9, 33), 21)
  want, want_hist, ws = run(images)
  assert np.array_equal(want_hist.cpu().numpy().astype(np.uint32), R.batch(images)[1])
  state = torch.tensor([4, 10], dtype=torch.int32, device=DEV)
  # the same workspace again and again, never zeroed by the host in between
  sc, _, _ = run(images, capacity=6, cursor=state[0:1], dropped=state[1:2], ws=ws)
  assert state.tolist() == [7, 11]
  assert torch.equal(bits(sc[4:6]), bits(want[0:2])) and bool((sc[:4] == SENTINEL).all())
  sc, _, _ = run(images, capacity=6, cursor=state[0:1], dropped=state[1:2], ws=ws)
  assert state.tolist() == [10, 14] and bool((sc == SENTINEL).all())
  sc, hist, _ = run(images, capacity=2, dropped=state[1:2], ws=ws)                  # no cursor: rows 0, 1; the third is dropped
  assert state.tolist() == [10, 15] and torch.equal(bits(sc), bits(want[0:2]))
  assert torch.equal(hist, want_hist), "hist is indexed by the image, not by the cursor"
  sc, hist, _ = run(images * 0.5, ws=ws, want_hist=False)
  assert bool((hist == HSENT).all())
  assert bool((R.ulp_gap(sc.cpu().numpy(), R.batch(images * 0.5)[0]) <= 1.0).all())


def test_error_returns_write_nothing():
  lib = nat.load()
  x = torch.full((2, 1, 4, 5), 0.5, device=DEV)
  sc = torch.full((2, 2), SENTINEL, device=DEV)
  hist = torch.full((2, 2, 256), HSENT, dtype=torch.int32, device=DEV)
  state = torch.tensor([3, 5], dtype=torch.int32, device=DEV)
  ws = workspace(2)
  def call(img=x, B=2, C=1, H=4, W=5, scores=sc, capacity=2, w=ws):
    return lib.as_image_entropy(nat.ptr(img), B, C, H, W, nat.ptr(scores), capacity, nat.ptr(state[0:1]), nat.ptr(state[1:2]),
                                nat.ptr(hist), nat.ptr(w), nat.stream())
  assert call(B=0) != 0 and call(B=65536) != 0 and b"65535" in lib.as_last_error()
  assert call(C=0) != 0 and call(H=0) != 0 and call(W=0) != 0 and call(capacity=0) != 0
  assert call(C=1 << 10, H=1 << 10, W=(1 << 10) + 1) != 0                  # C*H*W beyond 2^30
  assert call(img=None) != 0 and call(scores=None) != 0 and call(w=None) != 0
  assert lib.as_image_entropy_workspace(0) == 0 and lib.as_image_entropy_workspace(65536) == 0
  assert lib.as_image_entropy_workspace(2) >= 2 * (512 + 1) * 4
  torch.cuda.synchronize()
  assert bool((sc == SENTINEL).all()) and bool((hist == HSENT).all()) and state.tolist() == [3, 5] and not bool(ws.any())
  assert call() == 0
  torch.cuda.synchronize()
  assert state.tolist() == [5, 7] and bool((sc == SENTINEL).all())          # cursor 3 of capacity 2: both rows dropped


# ---- the collector -------------------------------------------------------------------------------------------------------------
def test_collector_appends_counts_drops_and_resets():
  batches = [torch.from_numpy(rand_images(s, i)).to(DEV) for i, s in enumerate(((2, 3, 9, 33), (3, 3, 9, 33), (2, 3, 9, 33)))]
  want = torch.cat([E.image_entropy(b) for b in batches])
  col = E.EntropyCollector(6, device=DEV)
  for b in batches:
    col.add(b)
  got = col.scores()
  assert got.shape == (6, 2) and torch.equal(bits(got), bits(want[:6])) and col.dropped() == 1
  col.reset()
  assert col.scores().shape == (0, 2) and col.dropped() == 0
  col.add(batches[1])
  assert torch.equal(bits(col.scores()), bits(want[2:5]))
  planes = batches[0][:, 0].contiguous()                                      # [B,H,W]
  torch.cuda.synchronize()
  before = torch.cuda.memory_allocated()
  col.add(batches[0])
  col.add(planes)
  assert torch.cuda.memory_allocated() == before, "add() allocated"
  with pytest.raises(RuntimeError, match="no CPU path"):
    col.add(batches[0].cpu())
  with pytest.raises(RuntimeError, match="contiguous fp32"):
    col.add(batches[0].transpose(2, 3))
  with pytest.raises(RuntimeError, match="no CPU path"):
    E.EntropyCollector(4, device="cpu")


def test_collector_in_a_captured_graph_appends_on_every_replay():
  shape = (2, 3, 9, 33)
  contents = [rand_images(shape, 40 + i) for i in range(3)]
  eager = [E.image_entropy(torch.from_numpy(c).to(DEV)) for c in contents]
  static = torch.from_numpy(contents[0]).to(DEV)
  col = E.EntropyCollector(5, device=DEV)
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    col.add(static)                                        # warm-up outside the capture: sizes the workspace
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
  assert got.shape == (5, 2) and col.dropped() == 1          # the cursor advanced 2, 4, 6: the sixth row did not fit
  assert torch.equal(bits(got), bits(torch.cat(eager)[:5]))


def test_collect_image_entropy_over_a_batch_list():
  left = torch.from_numpy(rand_images((5, 3, 12, 40), 77))
  batches = [{"color_l/0": left[i:i + 2], "color_r/0": left[i:i + 2]} for i in (0, 2, 4)]
  got = ood.collect_image_entropy(batches, num_images=5)
  want = R.batch(left.numpy())[0]
  assert got.shape == (5, 2) and got.is_cuda
  assert bool((R.ulp_gap(got.cpu().numpy(), want) <= 1.0).all())
  assert torch.equal(bits(ood.collect_image_entropy(batches, num_images=3)), bits(got[:3]))
  assert ood.collect_image_entropy([], 4).shape == (0, 2)
  pr = ood.precision_recall(got[:3, 0], got[3:, 0], num=10)                   # the OOD tools take the column as they take FCS
  assert pr["tp"].shape == (10,)


def test_functional_form_refuses_to_size_its_workspace_inside_a_capture():
  """image_entropy keeps one workspace per stream; made inside a capture it would belong to the graph's pool and outlive it."""
  x = torch.from_numpy(rand_images((2, 1, 9, 33), 3)).to(DEV)
  want = E.image_entropy(x)
  side = torch.cuda.Stream()
  E.release_workspaces()
  out = torch.zeros(2, 2, device=DEV)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
    out.zero_()
    with pytest.raises(RuntimeError, match="outside the capture"):
      E.image_entropy(x)
  with torch.cuda.stream(side):
    E.image_entropy(x)                                     # sizes the stream's workspace
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
    out.copy_(E.image_entropy(x))
  graph.replay(); graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(bits(out), bits(want))
  E.release_workspaces()
  assert torch.equal(bits(E.image_entropy(x)), bits(want))     # a fresh workspace after the release
