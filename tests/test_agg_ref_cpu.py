"""tests/agg_ref.py on the CPU: (a) every restatement against torch's float64 conv3d, batch_norm and autograd at 1e-12; (b) every
bound brackets a tap-by-tap fp32 accumulation and torch's fp32 convolution, and is below a tenth of what one dropped term at a
sentinel moves; (c) the restated plans against the library's host queries over a sweep, every tile of the weight gradient covered
three times, every voxel owned once by the agg3d units; (d) every deliberately wrong restatement is told apart by a named case."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import agg_ref as ar

F64 = torch.float64
SMALL = [(1, 1, 2, 63), (1, 1, 4, 32), (1, 2, 4, 33), (1, 3, 4, 33), (2, 3, 5, 32), (1, 2, 3, 120), (1, 1, 2, 189)]


def ncdhw(t):
  return t.permute(0, 4, 1, 2, 3).contiguous()


def cl(t):
  return t.permute(0, 2, 3, 4, 1).contiguous()


def close(got, ref, what, tol=1e-12):
  scale = max(1.0, float(ref.abs().max()))
  err = float((got.double() - ref.double()).abs().max())
  assert err <= tol * scale, "%s: %.3e against a scale of %.3e" % (what, err, scale)


# ----------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("geom", SMALL, ids=ar.geom_id)
def test_restatements_equal_float64_torch(geom):
  B, D, H, W = geom
  c = ar.random_case(geom)
  x = ncdhw(c["x"].double()).requires_grad_(True)
  w = c["w"].double().requires_grad_(True)
  b = c["b"].double().requires_grad_(True)
  z = F.conv3d(x, w, b, padding=1)
  z.backward(ncdhw(c["g"].double()))
  r = ar.forward(c["x"], c["w"], c["b"])
  close(r["z"], cl(z.detach()), "z")
  close(ar.data_gradient(c["g"], c["w"])["g_x"], cl(x.grad), "g_x")
  d0, b0 = ar.prior(False)
  wg, wa = ar.weight_gradient(c["x"], c["g"]), ar.weight_gradient(c["x"], c["g"], d0, b0)
  close(wg["dW"], w.grad, "dW"); close(wg["db"], b.grad, "db")
  close(wa["dW"], w.grad + d0.double(), "dW accumulate"); close(wa["db"], b.grad + b0.double(), "db accumulate")
  # the strip form restated strip by strip is the same convolution
  if ar.agg_plan(geom)["strips"] > 1:
    close(ar.strip_conv(c["x"], c["w"], c["b"], geom), r["z"], "strip by strip")
  # the previous BatchNorm still in partials: one fp64 partial per unit, merged, against F.batch_norm in train mode
  zp = c["x"].double()
  unit = ar.unit_of(geom).reshape(-1)
  P = ar.agg_plan(geom)["units"]
  v = zp.reshape(-1, 32)
  cnt = torch.bincount(unit, minlength=P).double()
  mean = torch.zeros(P, 32, dtype=F64).index_add_(0, unit, v) / cnt[:, None]
  m2 = torch.zeros(P, 32, dtype=F64).index_add_(0, unit, (v - mean[unit]) ** 2)
  st, _ = ar.merged_state(cnt, mean, m2, c["gamma"], c["beta"], c["rm"], c["rv"])
  rm, rv = c["rm"].double().clone(), c["rv"].double().clone()
  y = F.batch_norm(ncdhw(zp), rm, rv, c["gamma"].double(), c["beta"].double(), True, 0.1, 1e-5)
  a_ref = F.leaky_relu(y, 0.2)
  close(st["running_mean"], rm, "running_mean"); close(st["running_var"], rv, "running_var")
  r2 = ar.forward(c["x"], c["w"], c["b"], st["scale"], st["shift"])
  close(r2["a"], cl(a_ref), "a", 1e-11)
  close(r2["z"], cl(F.conv3d(a_ref, c["w"].double(), c["b"].double(), padding=1)), "z of the fused operand", 1e-11)
  # the eval epilogue
  r3 = ar.forward(c["x"], c["w"], c["b"], ep_scale=c["scale"], ep_shift=c["shift"])
  y3 = F.leaky_relu(z.detach() * c["scale"].double().reshape(1, 32, 1, 1, 1) + c["shift"].double().reshape(1, 32, 1, 1, 1), 0.2)
  close(r3["y"], cl(y3), "eval epilogue")


# ----------------------------------------------------------------------------- (b)
def _fma32(x, sc, sh):
  return (x.double() * sc.double() + sh.double()).float()      # the product is exact in fp64: one rounding


def _lrelu32(y):
  return torch.maximum(y, y * torch.tensor(0.2, dtype=torch.float32))


def _seen(bound, move):
  """the sentinel's term (1e4 |w[co]|, per output channel) is ten bounds at least in the channel it moves most and in three
  quarters of the 32 channels (a weight that happens to be tiny moves its channel by little: nothing to see there)"""
  ok = bound < 0.1 * move
  return bool(ok[int(move.argmax())]) and int(ok.sum()) >= 24


@pytest.mark.parametrize("geom", SMALL + [(3, 5, 9, 40)], ids=ar.geom_id)
def test_fp32_accumulations_stay_inside_every_bound(geom, capsys):
  c = ar.random_case(geom)
  worst = {}

  def see(name, got, ref, bound):
    r = ar.ratio(got, ref, bound)
    worst[name] = max(worst.get(name, 0.0), r)
    assert r <= 1.0, "%s %s: err / bound %.3g" % (ar.geom_id(geom), name, r)

  r = ar.forward(c["x"], c["w"], c["b"])
  see("z tap by tap", ar.conv_sum(ar.pad_operand(c["x"]), c["w"], c["b"], torch.float32), r["z"], r["e_z"])
  see("z torch fp32", cl(F.conv3d(ncdhw(c["x"]), c["w"], c["b"], padding=1)), r["z"], r["e_z"])
  dg = ar.data_gradient(c["g"], c["w"])
  see("g_x tap by tap", ar.conv_sum(ar.pad_operand(c["g"]), ar.transposed(c["w"]), None, torch.float32), dg["g_x"], dg["e_g_x"])
  see("g_x torch fp32", cl(F.conv_transpose3d(ncdhw(c["g"]), c["w"], None, padding=1)), dg["g_x"], dg["e_g_x"])
  # the fused operand: fma, then max(y, slope y); the by-product against its own bound
  ra = ar.forward(c["x"], c["w"], c["b"], c["scale"], c["shift"])
  a32 = _lrelu32(_fma32(c["x"], c["scale"], c["shift"]))
  see("a_out", a32, ra["a"], ra["e_a_out"])
  see("z fused tap by tap", ar.conv_sum(ar.pad_operand(a32), c["w"], c["b"], torch.float32), ra["z"], ra["e_z"])
  see("z fused torch fp32", cl(F.conv3d(ncdhw(a32), c["w"], c["b"], padding=1)), ra["z"], ra["e_z"])
  # the eval epilogue on an fp32 accumulator
  re = ar.forward(c["x"], c["w"], c["b"], ep_scale=c["scale"], ep_shift=c["shift"])
  acc = ar.conv_sum(ar.pad_operand(c["x"]), c["w"], c["b"], torch.float32)
  y32 = _fma32(acc, c["scale"], c["shift"])
  see("y", torch.where(y32 > 0, y32, y32 * torch.tensor(0.2, dtype=torch.float32)), re["y"], re["e_y"])
  # the weight gradient, with and without a prior value
  for acc_ in (0, 1):
    d0, b0 = ar.prior(False) if acc_ else (None, None)
    wg = ar.weight_gradient(c["x"], c["g"], d0, b0)
    dW, db = ar.wgrad_sum(c["x"], c["g"], torch.float32)
    if acc_:
      dW, db = dW + d0, db + b0
    see("dW", dW, wg["dW"], wg["e_dW"]); see("db", db, wg["db"], wg["e_db"])
  # teeth: one dropped term at a sentinel moves the output by ten bounds at least
  B, D, H, W = geom
  sent = torch.nonzero(c["x"].abs() == 1e4)
  assert sent.shape[0] >= 8
  wg = ar.weight_gradient(c["x"], c["g"])
  for bi, d, y, x, ci in sent.tolist():
    move = 1e4 * c["w"][:, ci, 1, 1, 1].double().abs()                     # the centre tap: the voxel the sentinel sits on
    assert _seen(r["e_z"][bi, d, y, x], move), "z: the bound cannot see the sentinel at %r" % ((bi, d, y, x, ci),)
    move = 1e4 * ar.transposed(c["w"])[:, ci, 1, 1, 1].double().abs()
    assert _seen(dg["e_g_x"][bi, d, y, x], move), "g_x: the bound cannot see the sentinel at %r" % ((bi, d, y, x, ci),)
    assert float(c["g"][bi, d, y, x, ci].abs()) == 1e4                     # g carries its sentinels on the same voxels
    assert float(wg["e_dW"][ci, ci, 1, 1, 1]) < 0.1 * 1e8 and float(wg["e_db"][ci]) < 0.1 * 1e4
  with capsys.disabled():
    print("\n  agg_ref bracketing %s: " % ar.geom_id(geom) + ", ".join("%s %.3f" % kv for kv in sorted(worst.items())))


def test_crafted_families_are_exact_in_fp32():
  """single tap: forward and data gradient are copies scaled by a power of two; small integers: every sum is a whole number below
  2^24; two impulses: sums of two exact products — the float64 value IS an fp32 number and an fp32 accumulation gives it bit for
  bit"""
  for geom in [(1, 1, 4, 32), (1, 3, 4, 33)]:
    c = ar.random_case(geom)
    for t in range(27):
      w = ar.tap_weights(t)
      for src, wt in ((c["x"], w), (c["g"], ar.transposed(w))):
        r = ar.conv_sum(ar.pad_operand(src), wt)
        assert bool(torch.equal(ar.conv_sum(ar.pad_operand(src), wt, None, torch.float32).double(), r)), (geom, t)
    i = ar.integer_case(geom)
    r = ar.conv_sum(ar.pad_operand(i["x"]), i["w"], i["b"])
    assert bool(torch.equal(ar.conv_sum(ar.pad_operand(i["x"]), i["w"], i["b"], torch.float32).double(), r))
    assert float(r.abs().max()) < 2 ** 24
  for geom in ar.WGRAD_EXACT_GEOMS:
    fams = [ar.integer_case(geom)] + [ar.impulse_case(geom, s) for s in ar.IMPULSE_SPOTS]
    for k, c in enumerate(fams):
      for acc in (0, 1):
        d0, b0 = ar.prior(True) if acc else (None, None)
        ref = ar.weight_gradient(c["x"], c["g"], d0, b0)
        dW, db = ar.wgrad_sum(c["x"], c["g"], torch.float32)
        if acc:
          dW, db = dW + d0, db + b0
        assert bool(torch.equal(dW.double(), ref["dW"])) and bool(torch.equal(db.double(), ref["db"])), (geom, k, acc)
        assert bool(torch.equal(ref["dW"].float().double(), ref["dW"]))
      if k > 0:
        assert int((c["g"].abs().sum(-1) > 0).sum()) == 2, (geom, k)          # two impulses on two different voxels


def test_impulses_sit_where_their_names_say():
  geom = (1, 169, 2, 63)
  tile = ar.wgrad_tile_of(geom)
  c = ar.impulse_case(geom, "extra")
  assert [int(tile[s]) for s in c["spots"]] == [168, 167]                  # the extra tile, the last chunk's tile
  geom = (1, 3, 4, 33)
  c = ar.impulse_case(geom, "seam")
  (b0, d0, y0, x0), (b1, d1, y1, x1) = c["spots"]
  assert y0 * 35 + x0 == 127 and y1 * 35 + x1 == 128 and int(tile.max()) == 168 and d0 == d1
  assert [int(ar.wgrad_tile_of(geom)[s]) for s in c["spots"]] == [2, 3]
  c = ar.impulse_case(geom, "planes")
  assert c["spots"][0][1] == 0 and c["spots"][1][1] == 2


# ----------------------------------------------------------------------------- (c)
def _lib():
  from adaptive_stereo import _native as nat
  return nat, nat.load()


def test_the_tables_follow_from_the_restated_plans():
  for geom, e in ar.AGG_GEOMS:
    p = ar.agg_plan(geom)
    assert p["strips"] == 1 and {k: p[k] for k in e} == e, (geom, p)
  for geom, e in ar.STRIP_GEOMS:
    p = ar.agg_plan(geom)
    assert (p["strips"], p["Ws"], ar.strip_origin(p, geom[3], p["strips"] - 1)[1]) == (e["strips"], e["Ws"], e["dupc"]), (geom, p)
    assert p["npos"] % 128 != 0                                            # every strip geometry has a shifted-back last tile
  for geom, (tiles, slabs) in ar.WGRAD_GEOMS:
    p = ar.wgrad_plan(geom)
    assert (p["tiles"], p["slabs"] if p["lds"] else 0) == (tiles, slabs), (geom, p)
  for geom, lds in ar.FIRST_GEN_GEOMS:
    assert ar.lds3d_ok(geom) == lds
  assert ar.agg_plan((1, 12, 24, 31)) is None and ar.agg_plan((1, 12, 900, 78)) is None


def test_restated_plans_equal_the_host_queries_over_a_sweep():
  nat, lib = _lib()
  from adaptive_stereo.hip_ops import Pcl, CONV3D_333
  out = (ctypes.c_int * 8)()
  widths = list(range(32, 201)) + [300, 400, 1242]
  ntiles_seen, planes_seen, n_ok = set(), set(), 0
  for W in widths:
    for H in range(2, 26):
      for D in range(1, 14):
        for B in range(1, 5):
          geom = (B, D, H, W)
          g = Pcl(B, D, H, W, 1, 1, 1)
          p = ar.agg_plan(geom)
          assert lib.as_agg3d_ok(g) == (1 if p else 0), geom
          if p:
            n_ok += 1
            assert lib.as_agg3d_parts(g) == p["grid"], geom
            assert lib.as_agg3d_plan(g, out) == 1 and list(out) == ar.plan_vector(p), (geom, list(out), p)
            planes_seen.add((H, W))
          else:
            assert lib.as_agg3d_plan(g, out) == 0, geom
          assert lib.as_conv32_stat_parts(g, g, CONV3D_333) == ar.stat_parts(geom), geom
          wp = ar.wgrad_plan(geom)
          assert lib.as_conv32_wgrad_segments(g, g, CONV3D_333) == wp["segments"], geom
          assert lib.as_conv32_wgrad_workspace(g, g, CONV3D_333) == wp["workspace"], geom
          assert wp["lds"] == (W + 2 <= 191 and (H - 1) * (W + 2) + W >= 128), geom
          if wp["lds"]:
            ntiles_seen.add(wp["tiles"])
  assert n_ok > 50000
  # the assignment: the restatement against the library block by block, and every (tile, kd) walked exactly once
  ci, ki, ei = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
  probe = sorted(t for t in ntiles_seen if t <= 400 or t % 7 == 0) + [t for g, (t, s) in ar.WGRAD_GEOMS if t]
  for ntiles in probe:
    nchunks = min(ntiles, ar.CAP)
    for blk in range(ar.wgrad_grid(nchunks)):
      ok = lib.as_conv3d_wgrad_lds_assignment(ntiles, nchunks, blk, ctypes.byref(ci), ctypes.byref(ki), ctypes.byref(ei))
      exp = ar.wgrad_assign(blk, ntiles, nchunks)
      assert (bool(ok), ki.value, ei.value) == (exp[0], exp[2], exp[3]) and (not ok or ci.value == exp[1]), (ntiles, blk)
    assert bool((ar.wgrad_coverage(ntiles, nchunks) == 1).all()), ntiles
  # every interior voxel is written, and counted once: overlapped strip columns count once
  for (H, W) in sorted(planes_seen):
    t = ar.plane_tiles((1, 1, H, W))
    assert bool((t["owner"] >= 0).all()) and bool((t["writes"] >= 1).all()), (H, W)
    p = ar.agg_plan((1, 1, H, W))
    assert int(t["owner"].max()) == p["tpp"] - 1
  for geom in [g for g, _ in ar.AGG_GEOMS + ar.STRIP_GEOMS]:
    B, D, H, W = geom
    pc = ar.partial_counts(geom)
    assert int(pc.sum()) == B * D * H * W and int((pc > 0).sum()) == ar.agg_plan(geom)["units"], geom


# ----------------------------------------------------------------------------- (d)
def _differs(mut_z, ref, bound):
  """beyond the bound somewhere (a NaN — a voxel never written — counts)"""
  return ar.ratio(mut_z, ref, bound) > 1.0


def _bits_differ(a, b):
  return not bool(torch.equal(a.double().nan_to_num(1e30), b.double().nan_to_num(1e30)))


def _caught(kind, mut):
  hits = []
  if kind == "conv":
    geom = (40, 7, 2, 63) if mut[0] == "stale_fourth" else (1, 3, 4, 33)
    if mut[0] == "stale_fourth":
      mut = ("stale_fourth", ar.agg_plan(geom)["seg_len"])
      assert mut[1] == 2
    else:
      c = ar.random_case(geom)
      r = ar.forward(c["x"], c["w"], c["b"])
      if _differs(ar.conv_sum(ar.pad_operand(c["x"].double()), c["w"], c["b"], mut=mut), r["z"], r["e_z"]):
        hits.append("random %s" % ar.geom_id(geom))
      w = ar.tap_weights(mut[1])
      if _bits_differ(ar.conv_sum(ar.pad_operand(c["x"]), w, mut=mut), ar.conv_sum(ar.pad_operand(c["x"]), w)):
        hits.append("single tap %d %s" % (mut[1], ar.geom_id(geom)))
    i = ar.integer_case(geom)
    if _bits_differ(ar.conv_sum(ar.pad_operand(i["x"]), i["w"], i["b"], torch.float32, mut=mut),
                    ar.conv_sum(ar.pad_operand(i["x"]), i["w"], i["b"], torch.float32)):
      hits.append("integers %s" % ar.geom_id(geom))
  elif kind == "unwritten":
    geom = (257, 1, 2, 63) if mut[0] == "skip_round" else (1, 1, 4, 32)
    i = ar.integer_case(geom)
    z = ar.conv_sum(ar.pad_operand(i["x"]), i["w"], i["b"], torch.float32)
    zm = ar.unwritten(z, geom, mut)
    if int(torch.isnan(zm).sum()) > 0 and _bits_differ(zm, z):
      hits.append("integers %s: %d elements never written" % (ar.geom_id(geom), int(torch.isnan(zm).sum())))
    if mut[0] == "no_shift_back":
      for g2, _ in ar.STRIP_GEOMS:
        assert bool(ar.plane_tiles(g2)["last"].any()), g2
  elif kind == "strip":
    geom = (1, 2, 3, 120)
    c = ar.random_case(geom)
    r = ar.forward(c["x"], c["w"], c["b"])
    if _differs(ar.strip_conv(c["x"], c["w"], c["b"], geom, mut), r["z"], r["e_z"]):
      hits.append("random %s" % ar.geom_id(geom))
    i = ar.integer_case(geom)
    if _bits_differ(ar.strip_conv(i["x"], i["w"], i["b"], geom, mut), ar.strip_conv(i["x"], i["w"], i["b"], geom)):
      hits.append("integers %s" % ar.geom_id(geom))
    assert not _bits_differ(ar.strip_conv(i["x"], i["w"], i["b"], geom), ar.conv_sum(ar.pad_operand(i["x"].double()), i["w"], i["b"]))
  elif kind == "owner":
    for geom in [(1, 2, 3, 120), (1, 2, 2, 156)]:
      a, b = ar.partial_counts(geom, mut), ar.partial_counts(geom)
      if not bool(torch.equal(a, b)):
        hits.append("partial counts %s" % ar.geom_id(geom))
      elif mut is not None:
        assert ar.strip_origin(ar.agg_plan(geom), geom[3], 1)[1] == 0          # no overlap: nothing to take
  elif kind == "halo":
    geom = (1, 3, 4, 33)
    c = ar.random_case(geom)
    r = ar.forward(c["x"], c["w"], c["b"], c["scale"], c["shift"])
    sh = c["shift"].double()
    leak = torch.where(sh > 0, sh, sh * 0.2)
    ap = ar.pad_operand(r["a"], fill=leak) if mut == "voxel" else ar.pad_operand(r["a"], plane_fill=leak)
    if _differs(ar.conv_sum(ap, c["w"], c["b"]), r["z"], r["e_z"]):
      hits.append("random %s, affine operand" % ar.geom_id(geom))
  elif kind == "wgrad":
    geom = (1, 169, 2, 63)
    for name, c in [("integers", ar.integer_case(geom)), ("two impulses, extra tile", ar.impulse_case(geom, "extra"))]:
      dW, db = ar.wgrad_sum(c["x"], c["g"])
      mW, mb = ar.wgrad_sum(c["x"], c["g"], mut=mut)
      if _bits_differ(mW, dW) or _bits_differ(mb, db):
        hits.append("%s %s" % (name, ar.geom_id(geom)))
    c = ar.random_case((1, 3, 4, 33))
    ref = ar.weight_gradient(c["x"], c["g"])
    mW, mb = ar.wgrad_sum(c["x"], c["g"], mut=mut)
    if _differs(mW, ref["dW"], ref["e_dW"]) or _differs(mb, ref["db"], ref["e_db"]):
      hits.append("random 1x3x4x33")
  return hits


@pytest.mark.parametrize("name", sorted(ar.MUTANTS))
def test_every_wrong_restatement_is_caught(name, capsys):
  kind, mut = ar.MUTANTS[name]
  hits = _caught(kind, mut)
  with capsys.disabled():
    print("\n  '%s' told apart by: %s" % (name, "; ".join(hits)))
  assert hits, "no case tells '%s' from the right restatement" % name


def test_the_right_restatement_is_not_caught():
  for kind, mut in [("conv", ("row_off", -1)), ("wgrad", None), ("owner", None), ("strip", None)]:
    assert _caught(kind, mut) == [], kind
