"""tests/wino_ref.py on the CPU: (a) the float64 restatements of the minimal-filtering launches against torch's float64
convolutions and autograd at 1e-12, and the restated tiling against a walk over the units; (b) the fp32 emulation in the kernels'
association inside every derived bound on the random (sentinel) and offset families, the worst err / bound printed; (c) the exact
integer cases reproduce float64 bit for bit in the fp32 emulation and their precondition holds; (d) the cases of
tests/test_gpu_wino_fp64.py, scaled down (the same H and W, a 64 times lower unit floor, grid 8), tell each of the twelve
MUTANTS from the right restatement: each exceeds a bound by more than a factor of two, breaks exactness or leaves a pixel
unwritten; (e) the share of elements undecided on a LeakyReLU branch is at most 1e-4 on every scaled case (the GPU file asserts
it again at its own shapes before it judges).  (d) is what keeps the GPU file from passing vacuously."""
import pytest
import torch
import torch.nn.functional as F

import wino_ref as wr

SCALE, GRID = 64, 8
F32 = torch.float32


def _nchw(t):
  return t.permute(0, 3, 1, 2)


def _close(a, b, what):
  scale = max(float(b.abs().max()), 1.0)
  err = float((a - b).abs().max())
  assert err <= 1e-12 * scale, "%s: %.3e against float64 torch (scale %.3e)" % (what, err, scale)


def _geoms(d):
  return wr.geometries(d, scale=SCALE)


ALL = [(g, d) for d in wr.DILATIONS for g in _geoms(d)]
IDS = ["%s-d%d" % (wr.geom_id(g), d) for g, d in ALL]


# ----------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("d", wr.DILATIONS)
@pytest.mark.parametrize("H,W", [(16, 64), (17, 65), (19, 127), (18, 129)])
def test_restatements_equal_float64_torch(H, W, d):
  B = 2
  g = torch.Generator().manual_seed(H * 1000 + W + d)
  x, gz = torch.randn(B, H, W, 32, generator=g), torch.randn(B, H, W, 32, generator=g)
  w, b = torch.randn(32, 32, 3, 3, generator=g) * 0.06, torch.randn(32, generator=g)
  x64 = _nchw(x.double()).clone().requires_grad_(True)
  w64 = w.double().clone().requires_grad_(True)
  z = F.conv2d(x64, w64, b.double(), padding=d, dilation=d)
  z.backward(_nchw(gz.double()))
  zr = z.detach().permute(0, 2, 3, 1)
  _close(wr.conv_direct(x, w, d) + b.double(), zr, "direct forward")
  _close(wr.conv_wino(x, w, d) + b.double(), zr, "minimal-filtering forward")
  gxr = x64.grad.permute(0, 2, 3, 1)
  _close(wr.conv_direct(gz, w, d, transposed=True), gxr, "direct data gradient")
  _close(wr.conv_wino(gz, w, d, transposed=True), gxr, "minimal-filtering data gradient")
  dWd, dbd = wr.wgrad_direct(x, gz, d)
  _close(dWd, w64.grad, "direct weight gradient")
  _close(dbd, gz.double().sum((0, 1, 2)), "bias gradient")
  for shifted in (True, False):
    dW, db, _ = wr.wgrad_wino(x, gz, d, shifted=shifted)
    _close(dW, w64.grad, "minimal-filtering weight gradient (shifted %s)" % shifted)
    _close(db, dbd, "bias gradient (shifted %s)" % shifted)


def test_element_wise_chains_equal_float64_autograd():
  g = torch.Generator().manual_seed(5)
  zp, sk = torch.randn(1, 4, 64, 32, generator=g).double().requires_grad_(True), torch.randn(1, 4, 64, 32, generator=g)
  st = wr._state(3, "cpu")
  a, _ = wr.act_chain(zp.detach().float(), sk, st["scale"], st["shift"], 0.2)
  sl = wr.f32(0.2)                                             # (the kernels receive the slope as a float)
  ref = F.leaky_relu(zp.detach().float().double() * st["scale"].double() + st["shift"].double(), sl) + sk.double()
  _close(a, ref, "a_out")
  # g_z: stage 3 of the BatchNorm backward with given coefficients
  ga, z = torch.randn(1, 4, 64, 32, generator=g), torch.randn(1, 4, 64, 32, generator=g)
  coef = torch.randn(96, generator=g)
  r = wr.gz_chain(ga, z, st["scale"], st["shift"], st["mean"], coef, 0.2)
  y = z.double() * st["scale"].double() + st["shift"].double()
  gy = torch.where(y > 0, ga.double(), sl * ga.double())
  ref = (gy - coef[:32].double() - (z.double() - st["mean"].double()) * coef[32:64].double()) * coef[64:].double()
  _close(r["g_z"], ref, "g_z")


@pytest.mark.parametrize("geom,d", ALL, ids=IDS)
def test_tiling_functions_agree_with_a_walk_over_the_units(geom, d):
  B, H, W = geom
  L = d.bit_length() - 1
  assert wr.pairs(H, d) == sum(-(-(-(-(H - r) // d)) // 2) for r in range(d))
  n = wr.units(B, H, W, d)
  assert n >= 2048 // SCALE and wr.units(B - 1, H, W, d) < 2048 // SCALE
  for shifted in (True, False):
    own, extra = wr.owner_map(B, H, W, d, GRID, shifted)
    assert extra is None and bool(torch.equal(own, wr.owner_map_loop(B, H, W, d, GRID, shifted)))
  assert sorted(wr.c0(t, d) + j * d for t in range(32) for j in (0, 1)) == list(range(64))
  assert all(wr.c0(t, d) == ((t >> L) << (L + 1)) | (t & (d - 1)) for t in range(32))
  ns = wr.nseg(W)
  assert sum(wr.seg_keep(s, W) for s in range(ns)) == W
  assert wr.seg_start(ns - 1, W) == W - 64 and wr.seg_start(ns - 1, W, False) == 64 * (ns - 1)


def test_issue_table_at_the_acceptance_floor():
  for d in wr.DILATIONS:
    g = wr.geometries(d)
    assert g[0] == (2048 // d, 2 * d, 64) and wr.units(*g[0], d) == 2048 and wr.units(g[0][0] - 1, 2 * d, 64, d) == 2048 - d
    # units not a multiple of the grid — except at d = 1, where the smallest batch of 3 x 65 gives 2048 exactly (37 x 127 and
    # 23 + d x 191 are the ragged ranges of that dilation)
    assert (wr.units(*g[1], d) % 512 != 0) == (d > 1) and wr.units(*g[3], d) % 512 != 0
    assert wr.seg_keep(0, 65) == 1 and wr.seg_keep(1, 129) == 1 and wr.seg_keep(0, 127) == 63 and wr.seg_keep(1, 192) == 64
    for (B, H, W) in g:
      assert wr.units(B, H, W, d) >= 2048 > wr.units(B - 1, H, W, d) and B * H * W * 128 <= 600e6


# ----------------------------------------------------------------------------- (b)
def _emu_moments(z32, own, grid):
  """fp32 shifted sums per lane group (8 per partial), Chan's merge in fp32, as the forward kernel's epilogue"""
  cnt, mean, m2 = torch.zeros(grid), torch.zeros(grid, 32), torch.zeros(grid, 32)
  flat, o = z32.reshape(-1, 32), own.reshape(-1)
  for k in range(grid):
    v = flat[o == k]
    rn, rmean, rm2 = torch.zeros(()), torch.zeros(32), torch.zeros(32)
    for q in range(8):
      c = v[q::8]
      if c.shape[0] == 0:
        continue
      n = torch.tensor(float(c.shape[0]))
      dd = c - c[0]
      s1, s2 = torch.zeros(32), torch.zeros(32)
      for i in range(dd.shape[0]):
        s1 = s1 + dd[i]
        s2 = s2 + dd[i] * dd[i]
      ml, m2l = c[0] + s1 / n, (s2 - s1 * s1 / n).clamp(min=0)
      tot, delta = rn + n, ml - rmean
      rmean = rmean + delta * (n / tot)
      rm2 = rm2 + (m2l + delta * delta * (rn * n / tot))
      rn = tot
    cnt[k], mean[k], m2[k] = rn, rmean, rm2
  return cnt, mean, m2


def _emu_sums(v32, own, grid):
  out = torch.zeros(grid, v32.shape[-1])
  flat, o = v32.reshape(-1, v32.shape[-1]), own.reshape(-1)
  for k in range(grid):
    out[k] = flat[o == k].sum(0)
  return out


@pytest.mark.parametrize("fam", ["random", "offset"])
def test_fp32_emulation_stays_inside_every_bound(fam, capsys):
  worst = {}

  def see(name, r):
    worst[name] = max(worst.get(name, 0.0), r)
    assert r <= 1.0, "%s: fp32 emulation err / bound %.3g" % (name, r)
  for geom, d in ALL:
    B, H, W = geom
    c = wr.case(geom, d, fam)
    sl, w = c["slope"], c["w"]
    # forward
    a32 = wr.act_chain(c["z_prev"], c["a_pp"], c["st_in"]["scale"], c["st_in"]["shift"], sl, F32)[0]
    a64, e_a = wr.act_chain(c["z_prev"], c["a_pp"], c["st_in"]["scale"], c["st_in"]["shift"], sl)
    see("a_out", wr.ratio(a32, a64, e_a))
    f = wr.forward_z(a32, w, c["b"], d)
    z32 = wr.conv_wino(a32, w, d, F32) + c["b"]
    see("z", wr.ratio(z32, f["z"], f["e_z"]))
    own, _ = wr.owner_map(B, H, W, d, GRID)
    m = wr.moments(z32, d, GRID)
    cnt, mean, m2 = _emu_moments(z32, own, GRID)
    assert bool(torch.equal(cnt.double(), m["cnt"]))
    see("mean", wr.ratio(mean, m["mean"], m["e_mean"]))
    see("M2", wr.ratio(m2, m["m2"], m["e_m2"]))
    # inference block
    e = wr.eval_out(c["x"], w, c["b"], c["st"]["scale"], c["st"]["shift"], sl, 1, d)
    y32 = (wr.conv_wino(c["x"], w, d, F32) + c["b"]) * c["st"]["scale"] + c["st"]["shift"]
    see("eval", wr.ratio(torch.maximum(y32, y32 * sl) + c["x"], e["out"], e["e_out"]))
    # data gradient
    st = c["st"]
    g32 = wr.gz_chain(c["g_a"], c["z"], st["scale"], st["shift"], st["mean"], c["coef"], sl, F32)["g_z"]
    r, und = wr.judge_gz(g32, wr.gz_chain(c["g_a"], c["z"], st["scale"], st["shift"], st["mean"], c["coef"], sl))
    see("g_z", r)
    dg = wr.data_gradient(g32, c["g_a"], w, d)
    gx32 = wr.conv_wino(g32, w, d, F32, transposed=True) + c["g_a"]
    see("g_x", wr.ratio(gx32, dg["g_x"], dg["e_g_x"]))
    sn = c["st_next"]
    ns = wr.next_sums(gx32, c["z_next"], sn["scale"], sn["shift"], sn["mean"], sl, d, GRID)
    yn = c["z_next"] * sn["scale"] + sn["shift"]
    gy = torch.where(yn > 0, gx32, gx32 * sl)
    emu = torch.cat([_emu_sums(gy, own, GRID), _emu_sums(gy * (c["z_next"] - sn["mean"]), own, GRID)], 1)
    see("next sums", wr.ratio(emu, ns["sums"], ns["e_sums"]))
    # weight gradient, both partitions
    for shifted, grid in ((False, GRID // 2), (True, GRID // 2)):
      wg = wr.weight_gradient(c["x"], g32, d, grid, shifted, slabs=grid)
      dW32, db32, _ = wr.wgrad_wino(c["x"], g32, d, F32, shifted=shifted)
      see("dW", wr.ratio(dW32, wg["dW"], wg["e_dW"]))
      see("db", wr.ratio(db32, wg["db"], wg["e_db"]))
  with capsys.disabled():
    print("\n  worst fp32-emulation err / bound (%s): %s" % (fam, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


# ----------------------------------------------------------------------------- (c)
def _exact_geoms():
  return [(g, d) for d in wr.DILATIONS for g in _geoms(d)[:3]]


@pytest.mark.parametrize("geom,d", _exact_geoms(), ids=["%s-d%d" % (wr.geom_id(g), d) for g, d in _exact_geoms()])
def test_exact_cases_are_exact_in_fp32(geom, d):
  for wfam in wr.EXACT_WEIGHTS[::3] + [wr.EXACT_WEIGHTS[-1]]:
    c = wr.exact_case(geom, d, wfam)
    sl, w, st = c["slope"], c["w"], c["st"]
    a32 = wr.act_chain(c["z_prev"], c["a_pp"], c["st_in"]["scale"], c["st_in"]["shift"], sl, F32)[0]
    assert bool(torch.equal(a32.double(), wr.act_chain(c["z_prev"], c["a_pp"], c["st_in"]["scale"], c["st_in"]["shift"], sl)[0]))
    assert bool(torch.equal(a32 * 4, (a32 * 4).round()))
    assert wr.exact_headroom(a32, w, d, 0.25, 1.0) < 2 ** 24
    assert bool(torch.equal((wr.conv_wino(a32, w, d, F32) + c["b"]).double(), wr.conv_direct(a32, w, d) + c["b"].double()))
    g32 = wr.gz_chain(c["g_a"], c["z"], st["scale"], st["shift"], st["mean"], c["coef"], sl, F32)["g_z"]
    assert bool(torch.equal(g32.double(), wr.gz_chain(c["g_a"], c["z"], st["scale"], st["shift"], st["mean"], c["coef"], sl)["g_z"]))
    assert bool(torch.equal(g32, g32.round()))
    assert wr.exact_headroom(g32, w, d, 1.0, 1.0, transposed=True) < 2 ** 24
    assert bool(torch.equal(wr.conv_wino(g32, w, d, F32, transposed=True).double(), wr.conv_direct(g32, w, d, transposed=True)))
    for shifted in (True, False):
      assert wr.exact_headroom_wgrad(c["x"], g32, d, 1.0, 1.0, shifted) < 2 ** 24
      dW32, db32, _ = wr.wgrad_wino(c["x"], g32, d, F32, shifted=shifted)
      dW, db = wr.wgrad_direct(c["x"], g32, d)
      assert bool(torch.equal(dW32.double(), dW)) and bool(torch.equal(db32.double(), db))


# ----------------------------------------------------------------------------- (d)
def _caught(mut_out, ref, bound):
  """a kernel making this mistake lands within `bound` of the mutant: it fails the test if the mutant is further than 2 x bound
  from the restatement somewhere, or leaves an element unwritten"""
  return wr.ratio(mut_out, ref, bound) > 2.0


def _conv_mutant_caught(mut, transposed):
  hit = []
  for geom, d in ALL:
    c = wr.case(geom, d, "random")
    x = c["g_a"] if transposed else c["x"]
    ref = wr.conv_direct(x, c["w"], d, transposed=transposed)
    S = wr.conv_wino(x.abs(), c["w"].abs(), d, transposed=transposed, absolute=True)
    if _caught(wr.conv_wino(x, c["w"], d, transposed=transposed, mut=mut, grid=GRID), ref, wr.gamma(wr.N_CONV) * S):
      hit.append((geom, d))
    ce = wr.exact_case(geom, d, ("dense", 0))
    xe = ce["g_a"] if transposed else ce["x"]
    if not bool(torch.equal(wr.conv_wino(xe, ce["w"], d, transposed=transposed, mut=mut, grid=GRID),
                            wr.conv_direct(xe, ce["w"], d, transposed=transposed))):
      hit.append((geom, d, "exact"))
  return hit


@pytest.mark.parametrize("num", [4, 5, 6, 7, 8, 9, 12])
def test_convolution_mutants_are_caught(num):
  hit = _conv_mutant_caught(wr.MUTANTS[num], False)
  assert hit, "mutant %d (%s) passes every case" % (num, wr.MUTANTS[num])
  if num in (6, 9):
    assert all(h[1] > 1 for h in hit)
  if num == 7:
    assert all(h[1] == 1 for h in hit)


def test_unmirrored_transposed_filter_is_caught():
  assert _conv_mutant_caught(wr.MUTANTS[10], True)
  assert not _conv_mutant_caught(wr.MUTANTS[10], False)          # (the forward filter has no mirror to forget)


def test_right_restatement_passes_its_own_mutant_criterion():
  assert not _conv_mutant_caught(None, False) and not _conv_mutant_caught(None, True)


def test_weight_gradient_mutants_are_caught():
  hits = {1: [], 11: [], 110: [], 12: []}
  for geom, d in ALL:
    c = wr.case(geom, d, "random")
    wg = wr.weight_gradient(c["x"], c["g_a"], d, GRID // 2, True, slabs=GRID // 2)
    for key, mut in ((1, "dw_unowned"), (11, ("g_quarter", 2)), (110, ("g_quarter", 0)), (12, "keep_mod")):
      dW, db, _ = wr.wgrad_wino(c["x"], c["g_a"], d, shifted=True, mut=mut)
      if _caught(dW, wg["dW"], wg["e_dW"]):
        hits[key].append((geom, d))
    assert not _caught(wr.wgrad_wino(c["x"], c["g_a"], d, shifted=True)[0], wg["dW"], wg["e_dW"])
  assert all(hits.values()), hits
  assert all(g[2] % 64 for g, _ in hits[1]) and all(g[2] % 64 == 0 for g, _ in hits[12])


def test_moment_and_sum_mutants_are_caught():
  hits = {2: [], 3: [], 12: []}
  for geom, d in ALL:
    B, H, W = geom
    c = wr.case(geom, d, "offset")
    sn = c["st_next"]
    m = wr.moments(c["x"], d, GRID)
    s = wr.next_sums(c["x"], c["z_next"], sn["scale"], sn["shift"], sn["mean"], 0.2, d, GRID)
    mm = wr.moments(c["x"], d, GRID, mut="mom_unowned")
    if not bool(torch.equal(mm["cnt"], m["cnt"])) and _caught(mm["mean"], m["mean"], m["e_mean"]):
      hits[2].append((geom, d))
    sm = wr.next_sums(c["x"], c["z_next"], sn["scale"], sn["shift"], sn["mean"], 0.2, d, GRID, mut="sums_unowned")
    if _caught(sm["sums"], s["sums"], s["e_sums"]):
      hits[3].append((geom, d))
    mk = wr.moments(c["x"], d, GRID, mut="keep_mod")
    sk = wr.next_sums(c["x"], c["z_next"], sn["scale"], sn["shift"], sn["mean"], 0.2, d, GRID, mut="keep_mod")
    if not bool(torch.equal(mk["cnt"], m["cnt"])) and _caught(sk["sums"], s["sums"], s["e_sums"]):
      hits[12].append((geom, d))
    assert float(m["cnt"].sum()) == B * H * W
  assert all(hits.values()), hits
  # every ragged geometry catches the double count, every dilation included
  assert {(g[2], d) for g, d in hits[2]} == {(g[2], d) for g, d in ALL if g[2] % 64} == {(g[2], d) for g, d in hits[3]}


def test_a_swap_of_two_pixels_between_partials_is_seen():
  """the gap of the merged comparison: one pixel counted twice, its neighbour missed — count and merged sums nearly unchanged"""
  geom, d = _geoms(1)[3], 1
  c = wr.case(geom, d, "offset")
  m = wr.moments(c["x"], d, GRID)
  z = c["x"].clone()
  z[0, 5, 70] = z[0, 5, 62]                                    # a shared column takes its neighbour's value
  assert wr.ratio(wr.moments(z, d, GRID)["mean"], m["mean"], m["e_mean"]) > 2.0


# ----------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("fam", ["random", "offset"])
def test_undecided_share_of_every_case_is_small(fam):
  for geom, d in ALL:
    c = wr.case(geom, d, fam)
    st, sn = c["st"], c["st_next"]
    r = wr.gz_chain(c["g_a"], c["z"], st["scale"], st["shift"], st["mean"], c["coef"], 0.2)
    n = c["z"].numel()
    assert int(r["undecided"].sum()) <= 1e-4 * n
    assert wr.next_sums(c["g_a"], c["z_next"], sn["scale"], sn["shift"], sn["mean"], 0.2, d, GRID)["undecided"] <= 1e-4 * n
