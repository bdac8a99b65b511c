"""tests/refine_ends_ref.py held to torch: every restatement against F.conv2d and float64 autograd of
relu(up + conv2d_out(lrelu(bn(z)) + skip)) and conv2d_feature at 1e-12 (relative to the largest value), an fp32 emulation of each
sum in the kernels' tap order bracketed by its bound, every MUTANT moved outside the bound (or to an unwritten / stray word) by
at least one geometry of the lists the GPU file runs, and the one condition that file relies on: the elements undecided on a
LeakyReLU branch, with the fixed seeds, are at most 1e-4 of a case and none where a case has fewer than 10^4 elements.  No GPU,
no library."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref as br
import refine_ends_ref as rr

F64 = torch.float64
SIZES = [(2, 5, 7), (1, 6, 8), (2, 13, 130), (1, 1, 1)]


def _close(got, ref, what, tol=1e-12):
  err = float((got.double() - ref.double()).abs().max()) / max(float(ref.double().abs().max()), 1.0)
  assert err <= tol, "%s: %.3e" % (what, err)


def _plain(geom, seed=0):
  """a case without sentinels, float64"""
  B, H, W = geom
  g = torch.Generator().manual_seed(1000 * seed + 7 * B + 131 * H + W)
  r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
  st, gamma = rr.state(5 + seed)
  return dict(z=r(B, H, W, 32), skip=r(B, H, W, 32), a=r(B, H, W, 32), g_a=r(B, H, W, 32), up=r(B, H, W), g_out=r(B, H, W),
              x4=r(B, H, W, 4), w_out=r(32, 9) * 0.2, b_out=r(1), w_in=r(32, 4, 3, 3) * 0.2, b_in=r(32),
              st={k: v.double() for k, v in st.items()}, gamma=gamma.double(), slope=0.2)


def _nchw(t):
  return t.permute(0, 3, 1, 2)


# ----------------------------------------------------------------------------- against torch
@pytest.mark.parametrize("geom", SIZES + [(2, 3, 62), (1, 4, 97)], ids=rr.geom_id)
def test_input_layer_against_conv2d_and_autograd(geom):
  c = _plain(geom)
  x = _nchw(c["x4"]).clone().requires_grad_(True)
  w, b = c["w_in"].clone().requires_grad_(True), c["b_in"].clone().requires_grad_(True)
  z = F.conv2d(x, w, b, padding=1)
  for pw in (1, 2, 8):
    _close(rr.conv4_sum(c["x4"], c["w_in"], c["b_in"], pw=pw), z.detach().permute(0, 2, 3, 1), "conv4 z, halo %d" % pw)
  gz = c["g_a"]
  z.backward(_nchw(gz))
  dW, db = rr.conv4_wgrad_sum(c["x4"], gz)
  _close(dW, w.grad, "conv4 dW")
  _close(db, b.grad, "conv4 db")
  # the disparity channel's data gradient: direct, and as nine projections + a gather
  _close(rr.g_up64(gz, c["w_in"], c["up"]), x.grad[:, 0] + c["up"], "g_up")
  _close(rr.tap_gather_sum(rr.proj_sum(gz, c["w_in"]), c["up"]), x.grad[:, 0] + c["up"], "g_up by projections")
  by_tap, by_ch = rr.mirror_taps_ch0(c["w_in"])
  assert torch.equal(by_tap.t(), by_ch) and float(by_ch[5, 2]) == float(c["w_in"][5, 0, 2, 0])


@pytest.mark.parametrize("geom", SIZES[:3] + [(1, 1, 2), (2, 13, 127), (2, 33, 5)], ids=rr.geom_id)    # (torch's BatchNorm wants two values)
def test_output_layer_and_the_block_before_it_against_autograd(geom):
  """relu(up + conv2d_out(lrelu(bn(z)) + skip)) with train-mode BatchNorm: a_out, out, g_pre, g_a, g_w, g_bias, the BatchNorm
  backward's sums and g_z"""
  c = _plain(geom, 1)
  B, H, W = geom
  z = _nchw(c["z"]).clone().requires_grad_(True)
  w = c["w_out"].t().reshape(1, 9, 32).permute(0, 2, 1).reshape(1, 32, 3, 3).clone().requires_grad_(True)
  b = c["b_out"].clone().requires_grad_(True)
  gamma, beta = c["gamma"], torch.randn(32, dtype=F64, generator=torch.Generator().manual_seed(3))
  y = F.batch_norm(z, None, None, gamma, beta, True, 0.0, br.EPS)
  a = F.leaky_relu(y, rr.f32(c["slope"])) + _nchw(c["skip"])          # (the kernels receive the slope as a float)
  a.retain_grad()
  out = F.relu(c["up"].unsqueeze(1) + F.conv2d(a, w, b, padding=1))
  out.backward(c["g_out"].unsqueeze(1))
  n, mean, m2 = br.moments64(c["z"])
  st = br.bn_state64(n, mean, m2, gamma, beta, torch.zeros(32), torch.ones(32))
  a_ref, _ = rr.act_chain(c["z"], c["skip"], st["scale"], st["shift"], c["slope"])
  _close(a_ref, a.detach().permute(0, 2, 3, 1), "a_out")
  for fn, kw in ((rr.refine_out_sum, dict(act=True)), (rr.refine_out_sum, dict(act=False)), (rr.thin_fwd_sum, {})):
    _close(fn(a_ref, c["w_out"], c["b_out"], c["up"], 1, **kw), out.detach()[:, 0], "out")
  g_pre = rr.relu_bwd(c["g_out"], out.detach()[:, 0])
  g_a, stray = rr.thin_dgrad_sum(g_pre, c["w_out"])
  assert stray == 0
  _close(g_a, a.grad.permute(0, 2, 3, 1), "g_a")
  g_w, g_b = rr.thin_wgrad_sum(a_ref, g_pre)
  _close(g_w, w.grad.reshape(32, 9), "g_w")
  _close(g_b, b.grad, "g_bias")
  coef = rr.bn_coef(g_a, c["z"], st, gamma, c["slope"])
  ref = rr.gz_chain(g_a, c["z"], st["scale"], st["shift"], st["mean"], coef, c["slope"])
  _close(ref["g_z"], z.grad.permute(0, 2, 3, 1), "g_z")
  for grid in (1, rr.bnsums_parts(B, H, W)):
    s = rr.bn_sums(g_a, c["z"], st["scale"], st["shift"], st["mean"], c["slope"], grid)
    full = br.bn_bwd64(g_a, c["z"], st, gamma, rr.f32(c["slope"]))
    _close(s["sums"].sum(0), torch.cat([full["sum_dy"], full["sum_dx"]]), "the slabs' total")


def test_small_launches():
  ch0, img = torch.randn(2, 3, 5), torch.randn(2, 3, 3, 5)
  x4 = rr.pack_in4(ch0, img)
  assert torch.equal(x4[..., 0], ch0) and torch.equal(x4[..., 1:], img.permute(0, 2, 3, 1))
  x3 = rr.pack_in4(None, img)
  assert torch.equal(x3[..., :3], img.permute(0, 2, 3, 1)) and float(x3[..., 3].abs().max()) == 0.0
  out = torch.tensor([1.0, 0.0, -0.0, -1.0, 1e-45])
  g = rr.relu_bwd(torch.tensor([2.0, 3.0, 4.0, 5.0, 6.0]), out)
  assert g.tolist() == [2.0, 0.0, 0.0, 0.0, 6.0] and not bool(torch.signbit(g).any())


@pytest.mark.parametrize("geom", [(1, 5, 100), (2, 3, 129), (3, 343, 5), (2, 2049, 3)], ids=rr.geom_id)
def test_chunk_ownership_is_the_kernels_loop(geom):
  for grid in (rr.bnsums_parts(*geom), rr.wgrad_grid(*geom), rr.dgrad_grid(*geom)):
    assert torch.equal(rr.chunk_owner(*geom, grid), rr.chunk_owner_loop(*geom, grid))


def test_routes_and_grids():
  assert rr.conv4_rows_route(62, 1, 1) and not rr.conv4_rows_route(61, 1, 1) and not rr.conv4_rows_route(31, 8, 8)
  assert rr.conv4_tiles(1, 1, 62) == (2, 1, 2)                   # waves 2 and 3 own no tile
  n, grid, _ = rr.conv4_tiles(1, 106, 1242)
  assert n == 4134 and grid == 1024                              # the tile loop strides
  assert rr.refine_out_ok(1, 0, 1, 1, 126) and not rr.refine_out_ok(1, 0, 1, 1, 125) and rr.refine_out_ok(1, 0, 8, 8, 1)
  assert rr.chunks(2, 2049, 3)[1] == 4098 and rr.wgrad_grid(2, 2049, 3) == 1024
  assert rr.chunks(4, 4097, 2)[1] == 16388 and rr.dgrad_grid(4, 4097, 2) == 16384
  assert rr.chunks(3, 343, 5)[1] == 1029 and rr.bnsums_parts(3, 343, 5) == 1024
  assert rr.ro_grid(2, 13, 127, False) == (2, 2, 8) and rr.ro_grid(2, 33, 253, True) == (3, 2, 12)


def test_own_column_mask_up_to_voxel_127_changes_no_word():
  """the issue's fourth refine_out mutant is value-neutral: column x0 + 126 is inside the image and the next strip's own"""
  for W in (1, 125, 126, 127, 253):
    a, b = rr.ro_a_out_writes(W), rr.ro_a_out_writes(W, 127)
    assert bool((a == 1).all()) and bool((b >= 1).all()) and int(b.sum() - a.sum()) == rr.cdiv(W, rr.RO_COLS) - 1


# ----------------------------------------------------------------------------- fp32 emulations inside the bounds
@pytest.mark.parametrize("geom", [(2, 13, 127), (2, 5, 65), (1, 4, 97)], ids=rr.geom_id)
def test_fp32_emulation_lies_inside_every_bound(geom):
  c = rr.case(geom)
  f32 = torch.float32
  inside = lambda got, ref, e, what: _assert_inside(rr.ratio(got, ref, e), what)
  f = rr.conv4_forward(c["x4"], c["w_in"], c["b_in"])
  inside(rr.conv4_sum(c["x4"], c["w_in"], c["b_in"], f32), f["z"], f["e_z"], "conv4 z")
  z32 = rr.conv4_sum(c["x4"], c["w_in"], c["b_in"], f32)
  y32 = z32 * c["st"]["scale"] + c["st"]["shift"]
  f1 = rr.conv4_forward(c["x4"], c["w_in"], c["b_in"], c["st"]["scale"], c["st"]["shift"], c["slope"])
  inside(torch.maximum(y32, y32 * c["slope"]), f1["z"], f1["e_z"], "conv4 epilogue 1")
  a_ref, e_a = rr.act_chain(c["z"], c["skip"], c["st"]["scale"], c["st"]["shift"], c["slope"])
  y = c["z"] * c["st"]["scale"] + c["st"]["shift"]
  a32 = torch.where(y > 0, y, y * c["slope"]) + c["skip"]
  inside(a32, a_ref, e_a, "a_out")
  o = rr.out_layer(a32, c["w_out"], c["b_out"], c["up"], 1)
  inside(rr.refine_out_sum(a32, c["w_out"], c["b_out"], c["up"], 1, dtype=f32), o["out"], o["e_out"], "out")
  g_pre = rr.relu_bwd(c["g_out"], c["out"])
  d = rr.data_gradient(g_pre, c["w_out"])
  ga32 = rr.thin_dgrad_sum(g_pre, c["w_out"], f32)[0]
  inside(ga32, d["g_a"], d["e_g_a"], "g_a")
  wg = rr.weight_gradient(c["a"], g_pre, c["g_w0"], c["g_b0"])
  gw32, gb32 = rr.thin_wgrad_sum(c["a"], g_pre, f32)
  inside(gw32 + c["g_w0"], wg["g_w"], wg["e_g_w"], "g_w")
  inside(gb32 + c["g_b0"], wg["g_b"], wg["e_g_b"], "g_bias")
  st = c["st"]
  grid = rr.bnsums_parts(*geom)
  s = rr.bn_sums(ga32, c["z"], st["scale"], st["shift"], st["mean"], c["slope"], grid)
  gy32 = torch.where(y > 0, ga32, ga32 * c["slope"])
  own = rr.chunk_owner(*geom, grid)
  emu = torch.cat([rr._slabs(gy32.double(), own, grid), rr._slabs((gy32 * (c["z"] - st["mean"])).double(), own, grid)], 1)
  inside(emu, s["sums"], s["e_sums"], "bnsums slabs")
  coef = rr.bn_coef(c["g_a"], c["z"], st, c["gamma"], c["slope"]).float()
  ref = rr.gz_chain(c["g_a"], c["z"], st["scale"], st["shift"], st["mean"], coef, c["slope"])
  k1, k2, k3 = coef[:32], coef[32:64], coef[64:]
  gy = torch.where(y > 0, c["g_a"], c["g_a"] * c["slope"])
  gz32 = (gy - k1 - (c["z"] - st["mean"]) * k2) * k3
  r, und = rr.judge_gz(gz32, ref)
  _assert_inside(r, "g_z")
  w4 = rr.conv4_weight_gradient(c["x4"], gz32, c["dW0"], c["db0"])
  dW32, db32 = rr.conv4_wgrad_sum(c["x4"], gz32, f32)
  inside(dW32 + c["dW0"], w4["dW"], w4["e_dW"], "conv4 dW")
  inside(db32 + c["db0"], w4["db"], w4["e_db"], "conv4 db")
  wp = rr.conv4_weight_gradient(c["x4"], ref["g_z"], None, None, rr.gz_bound(ref), rr.gz_both(ref))
  inside(dW32, wp["dW"], wp["e_dW"], "conv4 dW from the float64 chain")
  p = rr.proj_planes(ref, c["w_in"])
  h32 = rr.proj_sum(gz32, c["w_in"], f32)
  _assert_inside(rr.judge_h(h32, p), "h")
  t = rr.tap_gather(h32, g_pre)
  inside(rr.tap_gather_sum(h32, g_pre, f32), t["out"], t["e_out"], "tap gather")
  # composed: both routes to g_up inside the bound of the same float64 g_up
  up = rr.out_layer(gz32, rr.mirror_taps_ch0(c["w_in"])[1], None, g_pre, 0)
  inside(rr.tap_gather_sum(h32, g_pre, f32), up["out"], up["e_out"] + t["e_out"] + rr.tap_gather_sum(p["e_h"].abs()), "g_up by projections")


def _assert_inside(r, what):
  assert r <= 1.0, "%s: err / bound %.3g" % (what, r)


def test_exact_family_is_exact_in_fp32_with_headroom():
  geom = (2, 13, 127)
  room = 0.0
  for wfam in rr.EXACT_WEIGHTS:
    c = rr.exact_case(geom, wfam)
    f32 = torch.float32
    a, _ = rr.act_chain(c["z"], c["skip"], c["st"]["scale"], c["st"]["shift"], c["slope"])
    assert torch.equal(rr.refine_out_sum(a.float(), c["w_out"], c["b_out"], c["up"], 1, dtype=f32).double(),
                       rr.refine_out_sum(a, c["w_out"], c["b_out"], c["up"], 1))
    assert torch.equal(rr.conv4_sum(c["x4"], c["w_in"], c["b_in"], f32).double(), rr.conv4_sum(c["x4"], c["w_in"], c["b_in"]))
    room = max(room, rr.headroom(rr.out_layer(a.float(), c["w_out"], c["b_out"], c["up"], 0)["S"], rr.conv4_forward(c["x4"], c["w_in"], c["b_in"])["S"],
                                 rr.conv4_wgrad_sum(c["x4"].abs(), c["g_a"].abs())[0], rr.thin_wgrad_sum(a.abs(), c["g_out"].abs())[0]))
  assert room < 2 ** 24, room


# ----------------------------------------------------------------------------- the case lists tell the mutants apart
def _caught(got, ref, bound, stray=0):
  return stray > 0 or not rr.ratio(got, ref, bound) <= 1.0


def _try_mutant(mut, geom):
  """whether the GPU file's judgement of this geometry would reject a kernel that made the mutant's mistake"""
  c = rr.case(geom)
  B, H, W = geom
  st = c["st"]
  if mut.startswith("c4_"):
    f = rr.conv4_forward(c["x4"], c["w_in"], c["b_in"])
    return _caught(rr.conv4_sum(c["x4"], c["w_in"], c["b_in"], mut=mut), f["z"], f["e_z"])
  if mut.startswith("ro_"):
    for act in (True, False):
      o = rr.out_layer(c["a"], c["w_out"], c["b_out"], c["up"], 1)
      if _caught(rr.refine_out_sum(c["a"], c["w_out"], c["b_out"], c["up"], 1, act, mut=mut), o["out"], o["e_out"]):
        return True
    return False
  if mut.startswith("tf_"):
    ring = _ring(c["a"], geom)
    o = rr.out_layer(c["a"], c["w_out"], c["b_out"], c["up"], 1, ring=ring)
    return _caught(rr.thin_fwd_sum(c["a"], c["w_out"], c["b_out"], c["up"], 1, mut=mut, ring=ring), o["out"], o["e_out"])
  g_pre = rr.relu_bwd(c["g_out"], c["out"])
  if mut.startswith("tb_"):
    d = rr.data_gradient(g_pre, c["w_out"])
    g_a, stray = rr.thin_dgrad_sum(g_pre, c["w_out"], mut=mut)
    wg = rr.weight_gradient(c["a"], g_pre)
    return _caught(g_a, d["g_a"], d["e_g_a"], stray) or _caught(rr.thin_wgrad_sum(c["a"], g_pre, mut=mut)[0], wg["g_w"], wg["e_g_w"])
  if mut == "bs_contiguous":
    grid = rr.bnsums_parts(B, H, W)
    s = rr.bn_sums(c["g_a"], c["z"], st["scale"], st["shift"], st["mean"], c["slope"], grid)
    m = rr.bn_sums(c["g_a"], c["z"], st["scale"], st["shift"], st["mean"], c["slope"], grid, mut=mut)
    return _caught(m["sums"], s["sums"], s["e_sums"])
  coef = rr.bn_coef(c["g_a"], c["z"], st, c["gamma"], c["slope"]).float()
  ref = rr.gz_chain(c["g_a"], c["z"], st["scale"], st["shift"], st["mean"], coef, c["slope"])
  if mut == "pj_not_mirrored":
    p = rr.proj_planes(ref, c["w_in"])
    return not rr.judge_h(rr.proj_sum(ref["g_z"], c["w_in"], mut=mut), p) <= 1.0
  if mut == "tg_wrapped":
    h = rr.proj_sum(ref["g_z"], c["w_in"]).float()
    t = rr.tap_gather(h, g_pre)
    return _caught(rr.tap_gather_sum(h, g_pre, mut=mut), t["out"], t["e_out"])
  raise ValueError(mut)


def _ring(a, geom):
  """the image with data in the one-voxel border around it (the GPU file's non-zero-halo use of the thin forward)"""
  B, H, W = geom
  return torch.randn(B, H + 2, W + 2, 32, generator=torch.Generator().manual_seed(H * 1000 + W)).index_put_(
      (torch.arange(B).view(B, 1, 1), torch.arange(1, H + 1).view(1, H, 1), torch.arange(1, W + 1).view(1, 1, W)), a)


LISTS = {"c4_": rr.CONV4_ROWS[:-1], "ro_": rr.REFINE_OUT, "tf_": rr.THIN_FWD, "tb_": rr.THIN_BWD[:-1], "bs_": rr.BNSUMS,
         "pj_": rr.CONV4_WGRAD[:-1], "tg_": rr.TAP_GATHER}


@pytest.mark.parametrize("mut", sorted(rr.MUTANTS))
def test_every_mutant_is_caught_by_a_listed_geometry(mut):
  caught = [rr.geom_id(g) for g in LISTS[mut[:3]] if _try_mutant(mut, g)]
  print("mutant %s (%s): caught by %s" % (mut, rr.MUTANTS[mut], ", ".join(caught) or "NOTHING"))
  assert caught, "no listed geometry tells %s from the right restatement" % mut


# ----------------------------------------------------------------------------- the undecided-branch condition
UNDECIDED_CASES = sorted(set(rr.BNSUMS + rr.CONV4_WGRAD))


@pytest.mark.parametrize("geom", UNDECIDED_CASES, ids=rr.geom_id)
def test_undecided_elements_of_the_listed_cases_stay_under_the_cap(geom):
  c = rr.case(geom)
  st = c["st"]
  zs = c["z"].double() * st["scale"].double()
  y = zs + st["shift"].double()
  und = int((y.abs() <= rr.U * (1 + 2 * rr.U) * (zs.abs() + y.abs())).sum())
  n = c["z"].numel()
  print("undecided %s: %d of %d" % (rr.geom_id(geom), und, n))
  assert und <= 1e-4 * n and (n >= 10 ** 4 or und == 0)
