"""tests/lds2d_ref.py on the CPU: (a) the restated tiling — the owner map against a walk over the workgroups and their tiles,
the counts adding up to B H W — for every geometry of tests/test_gpu_lds2d_fp64.py; (b) the restated route decisions against the
library's read-only queries (as_conv32_stat_parts, as_conv32_bnbwd_parts, as_conv32_wgrad_workspace, as_conv32_wgrad_segments,
as_conv32_wgrad_bnapply_ok: host code, no GPU); (c) the float64 references and the tile-by-tile restatements against torch's
float64 convolutions and autograd at 1e-12; (d) each of the eight MUTANTS told from the right restatement: it exceeds a derived
bound by more than a factor of two, or changes a workgroup's count; (e) the elements undecided on a LeakyReLU branch, counted
for every case of the GPU file on its own operands, within 1e-4 of the case.  (d) keeps the GPU file from passing vacuously."""
import pytest
import torch
import torch.nn.functional as F

from adaptive_stereo import _native as nat
from adaptive_stereo.hip_ops import Pcl, ConvShape
import lds2d_ref as lr
import wino_ref as wr

ALL = lr.forward_cases()
EVERY = ALL + lr.WGRAD_LARGE + [lr.WGRAD_NARROW_HALO] + lr.BELOW_128
GEOMS = sorted(set(c[0] for c in ALL))


def _nchw(t):
  return t.permute(0, 3, 1, 2)


def _close(a, b, what):
  scale = max(float(b.abs().max()), 1.0)
  err = float((a - b).abs().max())
  assert err <= 1e-12 * scale, "%s: %.3e against float64 torch (scale %.3e)" % (what, err, scale)


# ----------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("geom", GEOMS, ids=[lr.geom_id(g) for g in GEOMS])
def test_owner_map_equals_a_walk_over_workgroups_and_tiles(geom):
  B, H, W = geom
  for grid in (lr.conv32_lds_grid(B, H, W), lr.conv32_wgrad_lds_slabs(B, H, W)):
    own, cover, cnt = lr.owner_map_loop(B, H, W, grid)
    assert bool(torch.equal(own, lr.owner_map(B, H, W, grid)))
    assert bool((cover == 1).all()) and int(cnt.sum()) == B * H * W
    assert bool(torch.equal(cnt, torch.bincount(own.reshape(-1), minlength=grid)))
    nt = lr.ntiles(B, H, W)
    walked = sorted(t for b in range(grid) for t in lr.wg_tiles(b, nt, grid))
    assert walked == list(range(nt)), "every tile is walked once"
    assert all(lr.wg_of_tile(t, nt, grid) == b for b in range(grid) for t in lr.wg_tiles(b, nt, grid))


def test_the_geometries_reach_the_edges_they_are_there_for():
  own, _, cnt = lr.owner_map_loop(1, 3, 128, 8)
  assert lr.conv32_lds_grid(1, 3, 128) == 8 and cnt.tolist() == [128, 128, 128, 0, 0, 0, 0, 0]
  assert lr.tile_coords(1, 5, 129) == (0, 0, 1, 128)                       # shifted to x0 = 1, one column of its own
  _, _, x0, x_new = lr.tile_coords(1, 9, 160)
  assert x_new - (x0 + 32 * 2) == 32 and x_new - (x0 + 32 * 3) == 0        # wave 2's dup == 32: the duplicates end on a wave boundary
  assert lr.tile_coords(1, 7, 255)[3] - lr.tile_coords(1, 7, 255)[2] == 1
  assert lr.tile_coords(1, 6, 256)[2:] == (128, 128)
  assert lr.tiles_per_row(257) == 3 and lr.tile_coords(2, 2, 257) == (0, 0, 129, 256)
  nt, grid = lr.ntiles(3, 29, 770), lr.conv32_lds_grid(3, 29, 770)
  assert (nt, grid) == (609, 512) and lr.most_tiles(nt, grid) == 2
  assert min(len(lr.wg_tiles(b, nt, grid)) for b in range(grid)) == 1 and nt - 7 * lr.band(nt) < lr.band(nt)   # a short last band
  assert not lr.wgrad_lds2(1, 3071, 128) and lr.wgrad_lds2(3, 1024, 128) and lr.wgrad_lds2(4, 384, 129)
  assert lr.ntiles(4, 384, 129) == lr.LDS2_TILES and lr.most_tiles(3072, 256) == 12


# ----------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("c", EVERY + [lr._c4((2, 40, 256), 2, (1, 8)), lr._c4((2, 40, 256), 1, (1, 7)), lr._c4((1, 3072, 128), 1)],
                         ids=lambda c: lr.case_id(c))
def test_restated_routes_equal_the_library_queries(c):
  (B, H, W), d, hin, hout = c
  lib = nat.load()
  gin, gout, shape = Pcl(B, 1, H, W, 0, *hin), Pcl(B, 1, H, W, 0, *hout), ConvShape(1, 3, 3, 0, d, d, d, 1)
  assert lib.as_conv32_stat_parts(gin, gout, shape) == lr.stat_parts(B, H, W, d, hin)
  assert lib.as_conv32_bnbwd_parts(gin, gout, shape) == lr.bnbwd_parts(B, H, W, d, hin)
  assert lib.as_conv32_wgrad_bnapply_ok(gin, gout, shape) == lr.wgrad_bnapply_ok(B, H, W, d, hin, hout)
  if hin[0] < d:
    return                                                   # (the remaining queries refuse an input halo the taps leave)
  ws = lr.wgrad_workspace(B, H, W, d, hin, hout)
  seg = lib.as_conv32_wgrad_segments(gin, gout, shape)
  if ws is None:
    assert seg >= 1 and lib.as_conv32_wgrad_workspace(gin, gout, shape) % (9 * 1024 + 32) == 0
  else:
    assert seg == 0 and lib.as_conv32_wgrad_workspace(gin, gout, shape) == ws


# ----------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("d", (1, 2, 3, 4, 7, 8))
@pytest.mark.parametrize("H,W", [(3, 128), (5, 129), (2, 257)])
def test_references_and_restatements_equal_float64_torch(H, W, d):
  B = 2
  g = torch.Generator().manual_seed(H * 1000 + W + d)
  x, gz = torch.randn(B, H, W, 32, generator=g), torch.randn(B, H, W, 32, generator=g)
  w, b = torch.randn(32, 32, 3, 3, generator=g) * 0.06, torch.randn(32, generator=g)
  x64 = _nchw(x.double()).clone().requires_grad_(True)
  w64 = w.double().clone().requires_grad_(True)
  z = F.conv2d(x64, w64, b.double(), padding=d, dilation=d)
  z.backward(_nchw(gz.double()))
  zr, gxr = z.detach().permute(0, 2, 3, 1), x64.grad.permute(0, 2, 3, 1)
  _close(lr.forward_z(x, w, b, d)["z"], zr, "forward")
  _close(lr.conv_tiles(x, w, d) + b.double(), zr, "forward, tile by tile")
  _close(lr.forward_z(gz, w, None, d, residual=x, transposed=True)["z"], gxr + x.double(), "data gradient + residual")
  _close(lr.conv_tiles(gz, w, d, transposed=True), gxr, "data gradient, tile by tile")
  dW, db = lr.wgrad_tiles(x, gz, d)
  _close(dW, w64.grad, "weight gradient, tile by tile")
  _close(db, gz.double().sum((0, 1, 2)), "bias gradient, tile by tile")
  st = wr._state(7, "cpu")
  sl = wr.f32(0.2)
  for res, rt in ((None, None), (gz, gz), ("self", x)):
    ref = F.leaky_relu(zr * st["scale"].double() + st["shift"].double(), sl) + (rt.double() if rt is not None else 0.0)
    _close(lr.eval_out(x, w, b, st["scale"], st["shift"], 0.2, rt, d)["out"], ref, "inference block")
    _close(lr.eval_tiles(x, w, b, st["scale"], st["shift"], 0.2, res, d), ref, "inference block, tile by tile")


def test_partial_sums_equal_plain_loops():
  B, H, W = 1, 5, 129
  grid = lr.conv32_lds_grid(B, H, W)
  g = torch.Generator().manual_seed(11)
  z, gx, zn = (torch.randn(B, H, W, 32, generator=g) for _ in range(3))
  own = lr.owner_map(B, H, W, grid)
  st = wr._state(5, "cpu")
  m = lr.moments(z, own, grid, 16)
  ns = lr.next_sums(gx, zn, st["scale"], st["shift"], st["mean"], 0.2, own, grid, 16)
  y = zn.double() * st["scale"].double() + st["shift"].double()
  gy = torch.where(y > 0, gx.double(), gx.double() * wr.f32(0.2))
  for k in range(grid):
    sel = own == k
    assert float(m["cnt"][k]) == float(sel.sum())
    if sel.any():
      _close(m["mean"][k], z[sel].double().mean(0), "mean of partial %d" % k)
      _close(m["m2"][k], ((z[sel].double() - z[sel].double().mean(0)) ** 2).sum(0), "M2 of partial %d" % k)
    _close(ns["sums"][k, :32], gy[sel].sum(0), "sum g_y of partial %d" % k)
    _close(ns["sums"][k, 32:], (gy[sel] * (zn[sel].double() - st["mean"].double())).sum(0), "sum g_y (z - mean) of partial %d" % k)
  flat = lr.flat_owner(B, H, W, 32)
  m = lr.moments_two_pass(z, flat, -(-B * H * W // 32))
  zz = z.double().reshape(-1, 32)
  _close(m["mean"][3], zz[96:128].mean(0), "flat partial mean")
  assert float(m["cnt"][-1]) == B * H * W - 32 * (m["cnt"].numel() - 1)


# ----------------------------------------------------------------------------- (d)
MUT_CASES = [lr._c4((1, 5, 129), 1), lr._c4((1, 9, 160), 2), lr._c4((2, 7, 255), 1), lr._c4((1, 2, 257), 4), lr._c4((1, 5, 129), 7)]


@pytest.mark.parametrize("c", MUT_CASES, ids=lambda c: lr.case_id(c))
def test_the_bounds_tell_the_arithmetic_mutants(c):
  """a dropped tap, the tap offset d - 1, the residual added before the activation, the skip from the wrong staged row, g_z
  not zeroed beyond W: each is off by more than twice the bound the GPU file applies; the right restatement is inside 1e-6 of it"""
  geom, d, _, _ = c
  k = lr.case(geom, d, "random")
  w, b, st = k["w"], k["b"], k["st"]
  f = lr.forward_z(k["x"], w, b, d)
  assert lr.ratio(lr.conv_tiles(k["x"], w, d) + b.double(), f["z"], f["e_z"]) < 1e-6
  for mut in ("drop_tap", "tap_dm1"):
    assert lr.ratio(lr.conv_tiles(k["x"], w, d, mut=mut) + b.double(), f["z"], f["e_z"]) > 2, mut
    gx = lr.forward_z(k["g_a"], w, None, d, residual=k["a_pp"], transposed=True)
    assert lr.ratio(lr.conv_tiles(k["g_a"], w, d, transposed=True, mut=mut) + k["a_pp"].double(), gx["z"], gx["e_z"]) > 2, mut
  for res, rt in ((k["a_pp"], k["a_pp"]), ("self", k["x"])):
    e = lr.eval_out(k["x"], w, b, st["scale"], st["shift"], k["slope"], rt, d)
    assert lr.ratio(lr.eval_tiles(k["x"], w, b, st["scale"], st["shift"], k["slope"], res, d), e["out"], e["e_out"]) < 1e-6
    assert lr.ratio(lr.eval_tiles(k["x"], w, b, st["scale"], st["shift"], k["slope"], res, d, mut="res_before_act"),
                    e["out"], e["e_out"]) > 2
  assert lr.ratio(lr.eval_tiles(k["x"], w, b, st["scale"], st["shift"], k["slope"], "self", d, mut="skip_row"), e["out"], e["e_out"]) > 2
  B, H, W = geom
  for route, slabs in (("lds", lr.conv32_wgrad_lds_slabs(B, H, W)), ("lds2", 256)):
    wg = lr.weight_gradient(k["x"], k["g_a"], d, route, slabs)
    dW, db = lr.wgrad_tiles(k["x"], k["g_a"], d)
    assert lr.ratio(dW, wg["dW"], wg["e_dW"]) < 1e-6 and lr.ratio(db, wg["db"], wg["e_db"]) < 1e-6
    if W % lr.SEG:
      dW, db = lr.wgrad_tiles(k["x"], k["g_a"], d, mut="g_wrapped")
      assert lr.ratio(dW, wg["dW"], wg["e_dW"]) > 2 and lr.ratio(db, wg["db"], wg["e_db"]) > 2


@pytest.mark.parametrize("geom", [(1, 5, 129), (1, 9, 160), (2, 7, 255), (1, 2, 257), (3, 29, 770)], ids=lr.geom_id)
def test_the_counts_and_sums_tell_the_tiling_mutants(geom):
  """the duplicate columns counted twice, dup off by one, a band boundary off by one: a workgroup's exact count changes, and
  its next-BatchNorm sums leave their bound"""
  B, H, W = geom
  grid = lr.conv32_lds_grid(B, H, W)
  _, _, cnt = lr.owner_map_loop(B, H, W, grid)
  k = lr.case(geom, 1, "random")
  sn = k["st_next"]
  n_l = 16 * lr.most_tiles(lr.ntiles(B, H, W), grid)
  ref = lr.next_sums(k["g_a"], k["z_next"], sn["scale"], sn["shift"], sn["mean"], 0.2, lr.owner_map(B, H, W, grid), grid, n_l)
  for mut in ("dup_twice", "dup_off_1", "band_off_1"):
    own, cover, c2 = lr.owner_map_loop(B, H, W, grid, mut)
    assert not bool(torch.equal(c2, cnt)), mut
    # the sums a kernel with this mistake would publish: every pixel weighted by how often (and by whom) it is counted
    if mut == "band_off_1":
      continue                                               # (two workgroups count one tile: the counts above show it)
    mutant = lr.next_sums(k["g_a"] * cover.unsqueeze(-1), k["z_next"], sn["scale"], sn["shift"], sn["mean"], 0.2,
                          own.clamp(min=0), grid, n_l)["sums"]
    assert lr.ratio(mutant, ref["sums"], ref["e_sums"]) > 2, mut


# ----------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("c", ALL + [lr.WGRAD_LARGE[2]], ids=lambda c: lr.case_id(c))
def test_undecided_elements_stay_within_the_cap(c):
  """on the GPU file's own operands: y_next of the MODE 3 launches (both bounded families), y of the APPLY launch"""
  geom, d, _, _ = c
  n = geom[0] * geom[1] * geom[2] * 32
  fams = ("random",) if c in lr.WGRAD_LARGE else ("random", "offset")
  for fam in fams:
    k = lr.case(geom, d, fam)
    if c in lr.WGRAD_LARGE:
      zs = k["z"].double() * k["st"]["scale"].double()
      y = zs + k["st"]["shift"].double()
      und = int((y.abs() <= lr.U * (1 + 2 * lr.U) * (zs.abs() + y.abs())).sum())
    else:
      und = lr.undecided_next(k["z_next"], k["st_next"]["scale"], k["st_next"]["shift"])
    assert und <= 1e-4 * n, "%s %s: %d of %d undecided" % (lr.case_id(c), fam, und, n)


def test_exact_cases_have_headroom():
  for c in lr.EXACT_CASES:
    geom, d, _, _ = c
    k = lr.exact_case(geom, d, ("dense", 0))
    room = lr.exact_headroom(lr.forward_z(k["x"], k["w"], k["b"], d)["S"] * 2 + 1,
                             lr.forward_z(k["g_a"], k["w"], None, d, residual=k["a_pp"], transposed=True)["S"],
                             *[2 * s + 8 for s in lr.wgrad_direct(k["x"].abs(), k["g_a"].abs(), d)])
    assert room < 2 ** 24, "%s: %.3g quanta" % (lr.case_id(c), room)
    z = lr.conv_tiles(k["x"], k["w"], d, dtype=torch.float32) + k["b"]
    assert bool(torch.equal(z.double(), lr.forward_z(k["x"], k["w"], k["b"], d)["z"])), "the fp32 evaluation is exact"
