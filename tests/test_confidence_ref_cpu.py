"""tests/confidence_ref.py on the CPU: the fp64 restatements of the confidence maps against torch's float64 soft-max and entropy
and against cases worked by hand; a float32 emulation of the written op order inside every bound on every case (the margin of
the bounds, shown on the reference alone); deliberately wrong restatements caught by the cases; the histogram at its bin edges;
the host halves of adaptive_stereo.confidence (curve, ause) on cases worked by hand; and the argument checks of the three entry
points, which return before any launch and so need no GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import confidence_ref as cr
import pointcloud_ref as pr
from adaptive_stereo import _native as nat
from adaptive_stereo import confidence as conf_mod

F = np.float32
CASES = [(shape, gain) for shape in cr.SHAPES for gain in cr.GAINS]
IDS = [cr.case_name(s, g) for s, g in CASES]


def _column(values):
  return np.asarray(values, F).reshape(1, -1, 1, 1)


# ---- the restatements ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,gain", CASES, ids=IDS)
def test_maps_agree_with_torch_softmax_in_float64(shape, gain):
  vol = cr.make_volume(shape, gain)
  r = cr.maps(vol)
  B, D, H, W = shape
  good = ~r["bad"]
  l = torch.from_numpy(vol).double()
  p = torch.softmax(l, dim=1)
  logp = torch.log_softmax(l, dim=1)
  ent = -(torch.where(p > 0, p * logp, torch.zeros_like(p))).sum(1).numpy()
  pmax = p.max(1)[0].numpy()
  am = torch.argmax(l, dim=1).numpy()
  assert np.array_equal(r["a"][good], am[good])                              # torch's argmax is the first maximum, too
  near = torch.zeros_like(p[:, 0])
  for k in (-1, 0, 1):
    i = torch.from_numpy(r["a"]) + k
    ok = (i >= 0) & (i < D)
    near = near + torch.where(ok, torch.gather(p, 1, i.clamp(0, D - 1)[:, None])[:, 0], torch.zeros_like(near))
  assert np.allclose(r["pmax"][good], pmax[good], rtol=1e-12, atol=0)
  assert np.allclose(r["mass"][good], near.numpy()[good], rtol=1e-12, atol=0)
  if D > 1:
    assert np.allclose(r["cent"][good], np.clip(1.0 - ent / math.log(D), 0, 1)[good], rtol=0, atol=1e-12)
  else:
    assert (r["cent"][good] == 1).all() and (r["pmax"][good] == 1).all() and (r["mass"][good] == 1).all()
  for k in cr.MAP_NAMES:
    assert np.isnan(r[k][~good]).all() and not np.isnan(r[k][good]).any()
    assert (r[k][good] >= 0).all() and (r[k][good] <= 1 + 1e-15).all()
  # the planted columns are where they should be and are what their names say
  where = cr.planted(shape)
  flat = {k: r[k].reshape(B, -1) for k in cr.MAP_NAMES + ("a", "bad")}
  for kind, (b, pix) in where.items():
    assert bool(flat["bad"][b, pix]) == (kind in cr.BAD_KINDS), kind
  if "max_both_ends" in where:
    assert flat["a"][where["max_both_ends"]] == 0
  if "mode_last" in where:
    assert flat["a"][where["mode_last"]] == D - 1
  if "all_equal" in where:
    b, pix = where["all_equal"]
    assert flat["a"][b, pix] == 0 and abs(flat["pmax"][b, pix] - 1.0 / D) < 1e-15 and abs(flat["mass"][b, pix] - 2.0 / D) < 1e-15
    assert flat["cent"][b, pix] < 1e-15
  if "one_hot_200" in where:
    assert all(abs(flat[k][where["one_hot_200"]] - 1.0) < 1e-15 for k in cr.MAP_NAMES)
  if "two_peaks" in where:
    assert flat["a"][where["two_peaks"]] == 1 and flat["pmax"][where["two_peaks"]] <= 0.5
  if "minus_inf" in where:
    assert 0 < flat["pmax"][where["minus_inf"]] <= 1


@pytest.mark.parametrize("D", [2, 3, 12, 24, 64])
def test_cases_worked_by_hand(D):
  r = cr.maps(_column([1.25] * D))                                           # uniform: 1/D, 0, 2/D (the window clipped at d = 0)
  assert abs(r["pmax"].item() - 1.0 / D) < 1e-15 and abs(r["cent"].item()) < 1e-15 and abs(r["mass"].item() - 2.0 / D) < 1e-15
  hot = [0.0] * D
  hot[D // 3] = 200.0
  r = cr.maps(_column(hot))                                                  # one-hot: 1, 1, 1
  assert all(abs(r[k].item() - 1.0) < 1e-15 for k in cr.MAP_NAMES)
  if D >= 4:
    two = [-300.0] * D
    two[1] = two[1 + D // 2] = 5.0
    r = cr.maps(_column(two))                                                # two equal far peaks: 0.5, 1 - ln 2 / ln D, 0.5
    assert abs(r["pmax"].item() - 0.5) < 1e-15 and abs(r["mass"].item() - 0.5) < 1e-15 and r["a"].item() == 1
    assert abs(r["cent"].item() - (1.0 - math.log(2.0) / math.log(D))) < 1e-15


def test_bad_columns_and_one_disparity():
  nan_bits = lambda v: np.asarray(v, F).view(np.uint32).item()
  for col in ([1.0, np.nan, 0.0], [np.inf, 0.0], [-np.inf] * 3, [np.nan], [np.inf], [-np.inf]):
    s = cr.stage(_column(col))
    assert s["bad"].item() and all(nan_bits(s[k]) == cr.QNAN_BITS for k in cr.MAP_NAMES), col
  s = cr.stage(_column([3.5]))
  assert all(s[k].item() == 1.0 and s["e_" + k].item() == 0.0 for k in cr.MAP_NAMES)
  s = cr.stage(_column([0.0, -np.inf, 0.0]))                                 # a -inf among finite values: probability 0
  assert not s["bad"].item() and abs(s["pmax"].item() - 0.5) < 1e-15 and abs(s["mass"].item() - 0.5) < 1e-15
  assert abs(s["cent"].item() - (1 - math.log(2) / math.log(3))) < 1e-15 and all(np.isfinite(s["e_" + k]).all() for k in cr.MAP_NAMES)


# ---- the bounds bracket a float32 run of the written op order ---------------------------------------------------------------
def _exp32(t):
  return torch.exp(torch.from_numpy(np.ascontiguousarray(t, dtype=F))).numpy()


def _log32(t):
  return torch.log(torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=F)))).numpy()


@pytest.mark.parametrize("shape,gain", CASES, ids=IDS)
def test_float32_emulation_lies_inside_every_bound(shape, gain):
  vol = cr.make_volume(shape, gain)
  s = cr.stage(vol)
  for name, (exp, log) in (("numpy", (np.exp, np.log)), ("torch", (_exp32, _log32))):
    got = cr.maps(vol, np.float32, exp=exp, log=log)
    assert np.array_equal(got["a"], s["a"])
    for k in cr.MAP_NAMES:
      ratio = cr.worst_ratio(got[k], s[k], s["e_" + k], s["bad"])
      print("%s %s %s: worst |err| / bound %.3f" % (cr.case_name(shape, gain), name, k, ratio))
      assert ratio <= 1.0, (name, k, ratio)


@pytest.mark.parametrize("what", sorted(cr.MUTANTS))
def test_wrong_restatements_are_caught(what):
  mut = cr.MUTANTS[what]
  caught = []
  for shape, gain in CASES:
    vol = cr.make_volume(shape, gain)
    s = cr.stage(vol)
    with np.errstate(all="ignore"):
      got = cr.maps(vol, np.float64, mut=mut)
    worst = max(cr.worst_ratio(got[k], s[k], s["e_" + k], s["bad"]) for k in cr.MAP_NAMES)
    if worst > 1.0:
      caught.append(cr.case_name(shape, gain))
  assert caught, "no case tells '%s' from the contract" % what
  print("%s: caught by %d of %d cases" % (what, len(caught), len(CASES)))


# ---- the gate -----------------------------------------------------------------------------------------------------------------
def test_gate_reference_at_its_edges():
  cam = pr.camera_constants(721.5, 743.1, 3.1, 2.2, 0.54, 0)
  disp = np.full((2, 1, 2, 4), 20.0, F)
  disp[1, 0, 1, 3] = 0.0                                                     # depth 100 > depth_trunc: invalid by depth
  p = pr.points(disp, cam, 0)
  cmin = F(0.3)
  conf = np.full((2, 2, 4), 0.5, F)
  conf[0, 0, 0] = cmin                                                       # kept
  conf[0, 0, 1] = np.nextafter(cmin, F(0), dtype=F)                          # rejected
  conf[0, 0, 2] = np.nan                                                     # rejected
  conf[0, 0, 3] = np.inf                                                     # kept
  conf[1, 1, 3] = 0.0                                                        # below, but invalid by depth anyway: not counted
  conf[1, 0, 0] = 0.0
  q, rejected = cr.gate(p, conf, cmin)
  assert rejected.tolist() == [2, 1]
  assert q["valid"][0, 0].tolist() == [True, False, False, True] and not q["valid"][1, 1, 3] and not q["valid"][1, 0, 0]
  assert p["valid"].sum() == 15 and q["valid"].sum() == 12                   # the input dict is left alone
  xyz = pr.organized(q)
  assert np.isnan(xyz[0, :, 0, 1]).all() and not np.isnan(xyz[0, :, 0, 0]).any()
  assert pr.voxel_cloud(q, 0, 0.15)["count"].sum() == 6
  q, rejected = cr.gate(p, conf, -np.inf)                                    # -inf keeps every number, not a NaN
  assert rejected.tolist() == [1, 0]


# ---- the histogram ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", cr.SPARSE_K)
def test_histogram_at_the_bin_edges(K):
  edges = (np.arange(K + 1, dtype=np.float64) / K).astype(F)
  below = cr._below(edges)
  key = np.concatenate([edges, below, np.array([-0.25, 1.5, np.inf, -np.inf, np.nan, 0.5, 0.5, 0.5, 0.5], F)])
  n = key.size
  gt = np.full(n, 10.0, F)
  pred = np.full(n, 12.0, F)
  pred[-4], gt[-3], gt[-2], gt[-1] = np.nan, 0.0, -1.0, np.nan
  pred[0] = 13.0                                                             # err == tau exactly: not bad
  pred[1 % n] = 13.5
  got = cr.sparsify_loop(key, pred, gt, 0.0, cr.bin_scale(K, 0, 1), K, 3.0)
  want = np.zeros(K, np.int64)
  for k in range(K + 1):
    want[min(k, K - 1)] += 1                                                 # the key k / K opens bin k; 1.0 falls into the last
    want[max(k - 1, 0)] += 1                                                 # its neighbour below closes bin k - 1; below 0: bin 0
  want[0] += 2                                                               # -0.25 and -inf
  want[K - 1] += 2                                                           # 1.5 and +inf
  assert got["count"].tolist() == want.tolist() and got["skipped"] == 2      # the NaN key and the NaN prediction
  assert got["bad"].sum() == 1 and got["count"].sum() == n - 5
  assert abs(got["abs_err"].sum() - (2.0 * (n - 5) + 1.0 + 1.5)) < 1e-9


@pytest.mark.parametrize("n", cr.SPARSE_N)
def test_histogram_cases_hold_what_they_should(n):
  key, pred, gt = cr.sparsify_case(n, 256)
  got = cr.sparsify_loop(key, pred, gt, 0.0, cr.bin_scale(256, 0, 1), 256, 3.0)
  assert got["count"].sum() + got["skipped"] == int((gt > 0).sum()) >= 1
  if n >= 4099:
    assert got["skipped"] >= 100 and (got["count"] > 0).sum() >= 200 and 0 < got["bad"].sum() < got["count"].sum()
    assert (cr.abs_err_bound(n, got["abs_err"]) <= 1e-12 * got["abs_err"]).all()          # n 2^-53: far below an fp32 ulp of the sum


# ---- curve and ause -----------------------------------------------------------------------------------------------------------
def test_curve_and_ause_worked_by_hand():
  count, bad, err = [2, 0, 1, 1], [2, 0, 0, 0], [10.0, 0.0, 2.0, 1.0]
  frac, epe, d1 = conf_mod.sparsification_curve(count, bad, err, "low")
  assert frac.tolist() == [0.0, 0.5, 0.5, 0.75, 1.0] and epe.tolist() == [13.0 / 4, 1.5, 1.5, 1.0, 0.0]
  assert d1.tolist() == [0.5, 0.0, 0.0, 0.0, 0.0]
  f2, e2, _ = conf_mod.sparsification_curve(count, bad, err, "high")
  assert f2.tolist() == [0.0, 0.25, 0.5, 0.5, 1.0] and e2.tolist() == [13.0 / 4, 4.0, 5.0, 5.0, 0.0]
  for remove in ("low", "high"):
    for a, b in zip(conf_mod.sparsification_curve(count, bad, err, remove), cr.curve_loop(count, bad, err, remove)):
      assert np.allclose(a, b, rtol=1e-15, atol=0)
  low = (frac, epe, d1)
  assert conf_mod.ause(low, low) == 0.0
  area = 0.5 * (13.0 / 4 + 1.5) / 2 + 0.25 * (1.5 + 1.0) / 2 + 0.25 * 1.0 / 2
  assert abs(conf_mod.ause(low, (np.array([0.0, 1.0]), np.array([0.0, 0.0]))) - area) < 1e-15
  # nothing at all: zeros, no division
  z = conf_mod.sparsification_curve([0, 0], [0, 0], [0.0, 0.0])
  assert all(v.tolist() == [0.0, 0.0, 0.0] for v in z)
  with pytest.raises(ValueError):
    conf_mod.sparsification_curve(count, bad, err, "middle")
  with pytest.raises(ValueError):
    conf_mod.ause((np.zeros(1), np.zeros(1)), low)


def test_a_perfect_key_gives_a_non_increasing_curve_and_zero_ause():
  rs = np.random.RandomState(3)
  K, n = 64, 5000
  err = (rs.rand(n) * 40).astype(F)
  gt = np.full(n, 50.0, F)
  pred = (gt + err).astype(F)
  err = np.abs(pred - gt)
  scale = cr.bin_scale(K, 0, 40)
  oracle = cr.sparsify_loop(err, pred, gt, 0.0, scale, K, 3.0)               # the error itself as the key
  perfect = cr.sparsify_loop(F(40) - err, pred, gt, 0.0, scale, K, 3.0)      # a confidence that orders the pixels as their error
  hi = conf_mod.sparsification_curve(oracle["count"], oracle["bad"], oracle["abs_err"], "high")
  assert (np.diff(hi[1]) <= 1e-12).all() and (np.diff(hi[2]) <= 1e-12).all() and hi[1][0] > 15
  assert conf_mod.ause(hi, hi) == 0.0
  lo = conf_mod.sparsification_curve(perfect["count"], perfect["bad"], perfect["abs_err"], "low")
  assert (np.diff(lo[1]) <= 1e-12).all()
  assert abs(conf_mod.ause(lo, hi)) < 0.05 * hi[1][0]                         # the two binnings differ only inside a bin
  shuffled = cr.sparsify_loop(rs.permutation(err), pred, gt, 0.0, scale, K, 3.0)
  flat = conf_mod.sparsification_curve(shuffled["count"], shuffled["bad"], shuffled["abs_err"], "low")
  assert conf_mod.ause(flat, hi) > 0.3 * hi[1][0]                             # a key that knows nothing


# ---- argument checks: before any launch, so without a GPU ---------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_a_gpu():
  lib = nat.load()
  buf = (ctypes.c_double * 64)()
  p = ctypes.cast(buf, ctypes.c_void_p)
  for args, word in (((None, 1, 3, 2, 2, p, p, p), b"bad argument"), ((p, 0, 3, 2, 2, p, p, p), b"bad argument"),
                     ((p, 65536, 3, 2, 2, p, p, p), b"65535"), ((p, 1, 0, 2, 2, p, p, p), b"[1, 64]"),
                     ((p, 1, 65, 2, 2, p, p, p), b"[1, 64]"), ((p, 1, 3, 0, 2, p, p, p), b"bad argument"),
                     ((p, 1, 3, 2, 2, None, None, None), b"no output")):
    assert lib.as_disp_confidence(*(args + (None,))) == -1
    assert word in lib.as_last_error(), (args, lib.as_last_error())

  def sp(key=p, pred=p, gt=p, n=8, lo=0.0, scale=4.0, K=4, tau=3.0, count=p, bad=p, err=p, skipped=p):
    return lib.as_sparsification(key, pred, gt, n, lo, scale, K, tau, count, bad, err, skipped, None)
  for kw, word in ((dict(key=None), b"null"), (dict(skipped=None), b"null"), (dict(n=0), b"n 0"), (dict(K=0), b"K 0"),
                   (dict(K=1025), b"K 1025"), (dict(scale=0.0), b"scale"), (dict(scale=float("inf")), b"scale"),
                   (dict(scale=float("nan")), b"scale"), (dict(lo=float("nan")), b"lo"), (dict(lo=float("-inf")), b"lo"),
                   (dict(tau=float("nan")), b"tau"), (dict(count=ctypes.c_void_p(p.value + 4)), b"aligned")):
    assert sp(**kw) == -1
    assert word in lib.as_last_error(), (kw, lib.as_last_error())

  cam = nat.DepthCamera(389.6, 180.0, 185.0, 66.0, 10.0, 100.0, 100.0, 80.0)

  def gated(disp=p, conf=p, conf_min=0.5, B=1, s=2, depth=p, cam=cam, table=None, slots=0):
    return lib.as_disp_to_points_gated(disp, None, conf, conf_min, B, 23, 524, s, ctypes.byref(cam), depth, None, 0.15, table, slots,
                                       None, None)
  for kw, word in ((dict(conf=None), b"conf is required"), (dict(conf_min=float("nan")), b"NaN"), (dict(disp=None), b"bad argument"),
                   (dict(s=3), b"bad argument"), (dict(depth=None), b"no output"),
                   (dict(cam=nat.DepthCamera(389.6, 180.0, 185.0, 66.0, 10.0, 700.0, 100.0, 80.0)), b"16-bit"),
                   (dict(table=ctypes.c_void_p(p.value & ~15), slots=512), b"slots")):
    assert gated(**kw) == -1
    assert b"as_disp_to_points_gated" in lib.as_last_error() and word in lib.as_last_error(), (kw, lib.as_last_error())


def test_python_layer_refuses_what_it_cannot_run():
  vol = torch.zeros(1, 3, 2, 2)
  with pytest.raises(RuntimeError, match="no CPU path"):
    conf_mod.disparity_confidence(vol)
  with pytest.raises(ValueError, match="kinds"):
    conf_mod.disparity_confidence(vol, kinds=("pmax", "variance"))
  with pytest.raises(ValueError, match="kinds"):
    conf_mod.disparity_confidence(vol, kinds=())
  with pytest.raises(RuntimeError, match="no CPU path"):
    conf_mod.upsample_confidence(torch.zeros(1, 2, 2), 4, 4)
  with pytest.raises(RuntimeError, match="no CPU path"):
    conf_mod.SparsificationCollector(device="cpu")
  for kw in (dict(bins=0), dict(bins=1025), dict(lo=1.0, hi=1.0), dict(hi=float("inf")), dict(tau=float("nan"))):
    with pytest.raises(ValueError):
      conf_mod.SparsificationCollector(device="cpu", **kw)
  assert conf_mod.bin_scale(256, 0.0, 1.0) == 256.0 and conf_mod.bin_scale(3, 0.0, 0.7) == float(cr.bin_scale(3, 0.0, 0.7))
