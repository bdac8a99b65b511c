"""tests/trunk_ref.py held to PyTorch on the CPU: the float64 restatement of the trunk's launches equals autograd on
torch.nn.functional to 1e-12, every bound brackets an fp32 emulation of the same sums added in another order (under the
bound, and above 1e-3 of it: a bound a thousand times too loose fails here), and the crafted-state cases of
tests/test_gpu_trunk_fp64.py have no ambiguous LeakyReLU branch."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref as br
import trunk_ref as tr


def _gen(seed):
  return torch.Generator().manual_seed(seed)


def _exact_state(z, gamma, beta, groups):
  zg = z.reshape(groups, -1, 32).double()
  mean = zg.mean(1)
  invstd = 1.0 / torch.sqrt(zg.var(1, unbiased=False) + br.EPS)
  scale = invstd * gamma.double()
  return dict(mean=mean, invstd=invstd, scale=scale, shift=beta.double() - mean * scale)


def _rel(a, b):
  return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def test_chain_equals_fp64_autograd():
  """two BasicBlocks and conv_alone from forward_layer, walked back with backward_layer and next_sums, against autograd on
  conv2d / batch_norm (train mode, the two groups as two calls) / leaky_relu in float64"""
  B, H, W, groups = 4, 5, 7, 2
  g = _gen(1)
  x0 = torch.randn(B, H, W, 32, generator=g, dtype=torch.float64)
  ws = [(torch.randn(32, 32, 3, 3, generator=g, dtype=torch.float64) / 17).requires_grad_() for _ in range(3)]
  bs = [(torch.randn(32, generator=g, dtype=torch.float64) * 0.1).requires_grad_() for _ in range(3)]
  gam = [(torch.rand(32, generator=g, dtype=torch.float64) + 0.5).requires_grad_() for _ in range(2)]
  bet = [torch.randn(32, generator=g, dtype=torch.float64).requires_grad_() for _ in range(2)]
  g_out = torch.randn(B, H, W, 32, generator=g, dtype=torch.float64)

  # torch
  a0 = x0.clone().requires_grad_()
  acts, zs_t = [a0], []
  for l in range(2):
    z = F.conv2d(acts[-1].permute(0, 3, 1, 2), ws[l], bs[l], padding=1)
    zs_t.append(z)
    per = B // groups
    y = torch.cat([F.batch_norm(z[i * per:(i + 1) * per], None, None, gam[l], bet[l], True, 0.1, br.EPS) for i in range(groups)])
    acts.append(F.leaky_relu(y, br.SLOPE).permute(0, 2, 3, 1) + acts[-1])
  out_t = F.conv2d(acts[-1].permute(0, 3, 1, 2), ws[2], bs[2], padding=1).permute(0, 2, 3, 1)
  (out_t * g_out).sum().backward()

  # the restatement: forward launches 0 (MODE 0), 1, 2 (MODE 1)
  with torch.no_grad():
    f0 = tr.forward_layer(x0, ws[0], bs[0])
    st0 = _exact_state(f0["z"], gam[0], bet[0], groups)
    f1 = tr.forward_layer(f0["z"], ws[1], bs[1], skip=x0, state=st0, groups=groups)
    st1 = _exact_state(f1["z"], gam[1], bet[1], groups)
    f2 = tr.forward_layer(f1["z"], ws[2], bs[2], skip=f1["a"], state=st1, groups=groups)
    assert _rel(f0["z"], zs_t[0].permute(0, 2, 3, 1)) < 1e-12 and _rel(f1["z"], zs_t[1].permute(0, 2, 3, 1)) < 1e-12
    assert _rel(f1["a"], acts[1]) < 1e-12 and _rel(f2["a"], acts[2]) < 1e-12 and _rel(f2["z"], out_t) < 1e-12
    # backward launches 2 (MODE 0: conv_alone), 1, 0 (MODE 1)
    b2 = tr.backward_layer(g_out, f2["a"], ws[2])
    s1 = tr.next_sums(b2["g_x"], f1["z"], st1, groups)
    b1 = tr.backward_layer(b2["g_x"], f1["a"], ws[1], z=f1["z"], state=st1, gamma=gam[1], groups=groups)
    s0 = tr.next_sums(b1["g_x"], f0["z"], st0, groups)
    b0 = tr.backward_layer(b1["g_x"], x0, ws[0], z=f0["z"], state=st0, gamma=gam[0], groups=groups)
    for l, b in ((2, b2), (1, b1), (0, b0)):
      assert _rel(b["dW"], ws[l].grad) < 1e-12, "dW of layer %d" % l
      # (the bias of a convolution in front of a BatchNorm has a zero gradient: relative to the sum of |terms|)
      assert float((b["db"] - bs[l].grad).abs().max()) < 1e-12 * float(b["g_z"].abs().reshape(-1, 32).sum(0).max()), \
          "db of layer %d" % l
    for l, b, s in ((1, b1, s1), (0, b0, s0)):
      assert _rel(b["g_gamma"].sum(0), gam[l].grad) < 1e-12 and _rel(b["g_beta"].sum(0), bet[l].grad) < 1e-12
      # the sums the launch above leaves are the ones this launch's BatchNorm backward is made of
      assert _rel(s["sum_dy"], b["g_beta"]) < 1e-12
      st = st1 if l == 1 else st0
      assert _rel(s["sum_dx"] * st["invstd"], b["g_gamma"]) < 1e-12
    assert _rel(b0["g_x"], a0.grad) < 1e-12
    assert f1["n_amb"] == 0 and f2["n_amb"] == 0 and b1["n_amb"] == 0 and b0["n_amb"] == 0


# ----------------------------------------------------------------------------- fp32 emulations in another order
def _conv32_reversed(a, w, bias):
  """z in float32: the 288 products of a voxel added one by one from the last tap and channel to the first, the bias last"""
  B, H, W, _ = a.shape
  ap = F.pad(a, (0, 0, 1, 1, 1, 1))
  acc = torch.zeros(B, H, W, 32, dtype=torch.float32)
  for kh in (2, 1, 0):
    for kw in (2, 1, 0):
      win = ap[:, kh:kh + H, kw:kw + W]
      for ci in range(31, -1, -1):
        acc = acc + win[..., ci:ci + 1] * w[:, ci, kh, kw]
  return acc + bias


def _dgrad32_reversed(g_z, w, res):
  B, H, W, _ = g_z.shape
  gp = F.pad(g_z, (0, 0, 1, 1, 1, 1))
  acc = torch.zeros(B, H, W, 32, dtype=torch.float32)
  for kh in (0, 1, 2):
    for kw in (0, 1, 2):
      win = gp[:, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W]      # g_z[y - kh + 1, x - kw + 1]
      for co in range(31, -1, -1):
        acc = acc + win[..., co:co + 1] * w[co, :, kh, kw]
  return acc + res if res is not None else acc


def _wgrad32_reversed(x, g_z):
  """dW, db in float32, one voxel at a time from the last to the first"""
  B, H, W, _ = x.shape
  xp = F.pad(x, (0, 0, 1, 1, 1, 1))
  dW = torch.zeros(32, 32, 3, 3, dtype=torch.float32)
  db = torch.zeros(32, dtype=torch.float32)
  for b in range(B - 1, -1, -1):
    for y in range(H - 1, -1, -1):
      for xx in range(W - 1, -1, -1):
        patch = xp[b, y:y + 3, xx:xx + 3]                      # [kh][kw][ci]
        dW = dW + g_z[b, y, xx][:, None, None, None] * patch.permute(2, 0, 1)[None]
        db = db + g_z[b, y, xx]
  return dW, db


def _bracket(name, got32, ref, bound, lo=1e-3):
  r = br.worst_ratio((got32.double() - ref).abs(), bound)
  assert r <= 1.0, "%s: the fp32 emulation is at %.3g of the bound" % (name, r)
  assert r >= lo, "%s: the fp32 emulation is at %.3g of the bound: the bound is too loose to test anything" % (name, r)
  return r


def _dense(B, H, W, groups, seed):
  g = _gen(seed)
  sc = tr.chan_scale()
  d = dict(src=torch.randn(B, H, W, 32, generator=g) * sc + 0.5 * sc, skip=torch.randn(B, H, W, 32, generator=g),
           g_a=torch.randn(B, H, W, 32, generator=g), x=torch.randn(B, H, W, 32, generator=g),
           z_next=torch.randn(B, H, W, 32, generator=g) * sc)
  d["gamma"] = torch.rand(32, generator=g) + 0.5
  d["beta"] = torch.randn(32, generator=g)
  d["w"], d["bias"] = tr.random_weights(seed + 5)
  return d


def _lrelu_two_roundings(src, scale, shift, slope):
  y = src * scale + shift
  return torch.where(y > 0, y, y * torch.tensor(slope, dtype=torch.float32))


def test_forward_bounds_bracket_an_fp32_emulation():
  """a (two roundings of the affine, slope, add) and z (288 products from the last to the first, then the bias) in float32
  against forward_layer: MODE 0 and MODE 1"""
  B, H, W, groups = 2, 6, 37, 2
  d = _dense(B, H, W, groups, 3)
  state, _ = tr.craft_state(d["src"], d["gamma"], groups, d["beta"])
  ref0 = tr.forward_layer(d["src"], d["w"], d["bias"])
  _bracket("z MODE 0", _conv32_reversed(d["src"], d["w"], d["bias"]), ref0["z"], ref0["e_z"])
  ref1 = tr.forward_layer(d["src"], d["w"], d["bias"], skip=d["skip"], state=state, groups=groups)
  assert ref1["n_amb"] == 0
  per = B // groups
  a32 = torch.cat([_lrelu_two_roundings(d["src"][i * per:(i + 1) * per], state["scale"][i], state["shift"][i], br.SLOPE)
                   for i in range(groups)]) + d["skip"]
  _bracket("a MODE 1", a32, ref1["a"], ref1["e_a"])
  _bracket("z MODE 1", _conv32_reversed(a32, d["w"], d["bias"]), ref1["z"], ref1["e_z"])


def _bwd32(d, state, groups, n_chunk):
  """the backward launch in float32: stage-1 sums in chunks of n_chunk voxels (fp32 inside a chunk, fp64 across: the kernel's
  lanes), stage 3, then the data and weight gradients from the last term to the first"""
  B = d["g_a"].shape[0]
  per = B // groups
  slope = torch.tensor(br.SLOPE, dtype=torch.float32)
  g_z = torch.empty_like(d["g_a"])
  for gi in range(groups):
    sl = slice(gi * per, (gi + 1) * per)
    ga, z = d["g_a"][sl].reshape(-1, 32), d["z"][sl].reshape(-1, 32)
    mean, invstd, scale, shift = (state[k][gi] for k in ("mean", "invstd", "scale", "shift"))
    y = (z.double() * scale.double() + shift.double()).float()
    g_y = torch.where(y > 0, ga, ga * slope)
    xc = z - mean
    N = ga.shape[0]
    sdy, sdx = torch.zeros(32, dtype=torch.float64), torch.zeros(32, dtype=torch.float64)
    for c0 in range(0, N, n_chunk):
      a, b = torch.zeros(32), torch.zeros(32)
      for i in range(min(N, c0 + n_chunk) - 1, c0 - 1, -1):
        a = a + g_y[i]
        b = b + g_y[i] * xc[i]
      sdy += a.double(); sdx += b.double()
    is64 = invstd.double()
    k1, k2, k3 = (sdy / N).float(), (sdx * is64 * is64 / N).float(), invstd * d["gamma"]
    g_z[sl] = ((g_y - k1 - xc * k2) * k3).reshape(d["g_a"][sl].shape)
  return g_z


def test_backward_bounds_bracket_an_fp32_emulation():
  """g_x, dW, db of MODE 0 and MODE 1, the BatchNorm parameter gradients and the sums for the layer below, in float32 in another
  order, against backward_layer / next_sums.

  MODE 1's g_x, dW and db carry two terms: the launch's own additions (`own_*`) and e_gz pushed through |w| or |x|.  e_gz is
  bn_ref.bwd_scales' worst case, K_BWD * n_lane = 256 roundings of the stage-1 terms on EVERY voxel with one sign, and a sum
  over N voxels adds it N times while independent roundings grow as sqrt(N): the emulation sits at 3e-3 of the whole bound
  of g_x and dW on this 42-voxel-per-group map and at 4e-4 .. 9e-4 of db's (db is a sum that cancels to zero) at any size
  tried.  So the two terms are bracketed where they arise: e_gz on g_z itself, the own term on an emulation fed with the
  reference's g_z rounded to fp32 (one more rounding per term: own * (1 + 1/n)), and the whole bound from above only."""
  B, H, W, groups = 2, 5, 37, 2
  d = _dense(B, H, W, groups, 4)
  # MODE 0
  ref0 = tr.backward_layer(d["g_a"], d["x"], d["w"])
  _bracket("g_x MODE 0", _dgrad32_reversed(d["g_a"], d["w"], None), ref0["g_x"], ref0["e_g_x"])
  dW32, db32 = _wgrad32_reversed(d["x"], d["g_a"])
  _bracket("dW MODE 0", dW32, ref0["dW"], ref0["e_dW"])
  _bracket("db MODE 0", db32, ref0["db"], ref0["e_db"])
  assert bool((ref0["e_gz"] == 0).all()) and torch.equal(ref0["own_dW"], ref0["e_dW"])
  # MODE 1
  B, H, W, groups = 4, 3, 7, 2
  N = B * H * W
  d = _dense(B, H, W, groups, 4)
  d["z"] = d["src"]
  n_lane = 16
  state, _ = tr.craft_state(d["z"], d["gamma"], groups, d["beta"])
  ref1 = tr.backward_layer(d["g_a"], d["x"], d["w"], z=d["z"], state=state, gamma=d["gamma"], groups=groups, n_lane=n_lane)
  assert ref1["n_amb"] == 0
  g_z32 = _bwd32(d, state, groups, n_lane)
  _bracket("g_z", g_z32, ref1["g_z"], ref1["e_gz"])
  gx32 = _dgrad32_reversed(g_z32, d["w"], d["g_a"])
  dW32, db32 = _wgrad32_reversed(d["x"], g_z32)
  for name, got in (("g_x", gx32), ("dW", dW32), ("db", db32)):
    _bracket(name + " MODE 1, whole bound", got, ref1[name], ref1["e_" + name], lo=0.0)
  g_zr = ref1["g_z"].float()
  dWr, dbr = _wgrad32_reversed(d["x"], g_zr)
  _bracket("g_x MODE 1, own term", _dgrad32_reversed(g_zr, d["w"], d["g_a"]), ref1["g_x"], ref1["own_g_x"] * (1 + 1 / 289))
  _bracket("dW MODE 1, own term", dWr, ref1["dW"], ref1["own_dW"] * (1 + 1 / N))
  _bracket("db MODE 1, own term", dbr, ref1["db"], ref1["own_db"] * (1 + 1 / N))
  # the sums for the layer below, from the g_x the emulation "stored"
  staten, _ = tr.craft_state(d["z_next"], d["gamma"], groups, d["beta"])
  refn = tr.next_sums(gx32, d["z_next"], staten, groups, n_lane)
  assert refn["n_amb"] == 0
  per = B // groups
  slope = torch.tensor(br.SLOPE, dtype=torch.float32)
  for gi in range(groups):
    gx, zn = gx32[gi * per:(gi + 1) * per].reshape(-1, 32), d["z_next"][gi * per:(gi + 1) * per].reshape(-1, 32)
    yn = zn * staten["scale"][gi] + staten["shift"][gi]
    gg = torch.where(yn > 0, gx, gx * slope)
    sdy, sdx = torch.zeros(32, dtype=torch.float64), torch.zeros(32, dtype=torch.float64)
    for c0 in range(0, gx.shape[0], n_lane):
      a, b = torch.zeros(32), torch.zeros(32)
      for i in range(min(gx.shape[0], c0 + n_lane) - 1, c0 - 1, -1):
        a = a + gg[i]
        b = b + gg[i] * (zn[i] - staten["mean"][gi])
      sdy += a.double(); sdx += b.double()
    _bracket("sum_dy group %d" % gi, sdy, refn["sum_dy"][gi], refn["e_sum_dy"][gi])
    _bracket("sum_dx group %d" % gi, sdx, refn["sum_dx"][gi], refn["e_sum_dx"][gi])
    # ... read back as this layer's parameter gradients
    refb = tr.backward_layer(gx32, d["x"], d["w"], z=d["z_next"], state=staten, gamma=d["gamma"], groups=groups, n_lane=n_lane)
    _bracket("g_beta group %d" % gi, sdy.float(), refb["g_beta"][gi], refb["e_g_beta"][gi])
    _bracket("g_gamma group %d" % gi, (sdx * staten["invstd"][gi].double()).float(), refb["g_gamma"][gi], refb["e_g_gamma"][gi])


def test_running_update_bound():
  """two sequential updates rounded to fp32 each stay within one ulp per update of the unrounded fp64 result, and the order
  of the groups shows when their means differ"""
  g = _gen(5)
  states = torch.randn(2, 5, 32, generator=g)
  states[1, 0] += 100.0
  states[:, 4] = states[:, 4].abs() + 0.1
  rm, rv = torch.randn(32, generator=g), torch.rand(32, generator=g) + 0.5
  m, v, e_m, e_v = tr.running_update(states, rm, rv, 0.1)
  mo = float(torch.tensor(0.1, dtype=torch.float32))
  m32, v32 = rm.double(), rv.double()
  for gi in range(2):
    m32 = (mo * states[gi, 0].double() + (1 - mo) * m32).float().double()
    v32 = (mo * states[gi, 4].double() + (1 - mo) * v32).float().double()
  assert bool(((m32 - m).abs() <= e_m).all()) and bool(((v32 - v).abs() <= e_v).all())
  assert br.worst_ratio((m32 - m).abs(), e_m) >= 1e-3
  mr, _, _, _ = tr.running_update(states.flip(0), rm, rv, 0.1)
  assert bool(((mr - m).abs() > 100 * e_m).all()), "the order of the groups must show"


def test_tiling_of_the_gpu_cases():
  """the geometry list covers what its comments say: dup 31, 20, 1, gper 72, 108 (two rounds) and 65 (uneven rounds)"""
  t = {tr.geom_id(g): tr.tiling(*g[:4]) for g in tr.GEOMS}
  assert [t[k]["dup"] for k in ("2x3x33_g2_h22", "2x9x44_g2_h13", "2x4x63_g2_h11")] == [31, 20, 1]
  assert t["2x24x78_g2_h11"]["gper"] == 72 and t["2x24x78_g2_h11"]["rounds"] == 1
  assert t["6x24x78_g2_h22"]["gper"] == 108 and t["6x24x78_g2_h22"]["rounds"] == 2
  assert t["1x43x96_g1_h13"]["gper"] == 65 and t["1x43x96_g1_h13"]["tiles_per_group"] == 129
  assert t["2x1x1_g2_h11"]["gper"] == 1 and t["3x6x16_g1_h11"]["gper"] == 18
  assert sorted({t[k]["gper"] for k in t}) == [1, 2, 3, 4, 6, 8, 9, 18, 65, 72, 108]


@pytest.mark.parametrize("geom", tr.GEOMS, ids=tr.geom_id)
def test_crafted_cases_have_no_ambiguous_branch(geom):
  """the seeds of the GPU file's crafted-state backward cases: no LeakyReLU branch of this layer or of the layer below depends
  on how y was rounded (the sums for the layer below are judged on the g_x the kernel stores; with a g_x of the reference the
  branch is the same, since it depends on z_next and the state alone)"""
  B, H, W, groups, _ = geom
  for fam in tr.BWD_FAMILIES:
    c = tr.bwd_case(fam, geom)
    st, _ = tr.craft_state(c["z"], c["gamma"], groups, c["beta"])
    stn, _ = tr.craft_state(c["z_next"], c["gamma_next"], groups, c["beta_next"])
    per = B // groups
    for gi in range(groups):
      sl = slice(gi * per, (gi + 1) * per)
      for z, s in ((c["z"], st), (c["z_next"], stn)):
        _, amb = br.lrelu_branch(z[sl], s["scale"][gi], s["shift"][gi])
        assert int(amb.sum()) == 0, "%s %s: %d ambiguous branches" % (tr.geom_id(geom), fam, int(amb.sum()))
