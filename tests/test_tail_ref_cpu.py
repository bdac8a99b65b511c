"""tests/tail_ref.py on the CPU: (a) the float64 restatements of the cost volume, the fused tail and its backward against torch's
float64 autograd (F.conv3d, softmax, sort); (b) a float32 emulation of each loop inside every derived bound on every committed
case, the worst err / bound printed — for the soft-argmax this is what shows K_EXP's margin on the reference alone; (c) the cases
discriminate: every deliberately wrong restatement of tail_ref.MUTANTS leaves a bound or breaks an exact family in at least one
committed case; (d) the case conditions that depend on the reference alone: the share of pixels whose arg-max is left undecided
stays below the cap in every case, and every geometry's route follows from the table's arithmetic.  (c) is what keeps
tests/test_gpu_tail_fp64.py from passing vacuously, and stands in on a machine without a GPU for reverting the last tile's
shift-back or swapping the backward's chunk width."""
import pytest
import torch
import torch.nn.functional as F

import tail_ref as tr

F64 = torch.float64


def _close(a, b, what, tol=1e-12):
  scale = max(float(b.abs().max()), 1.0)
  err = float((a.double() - b.double()).abs().max())
  assert err <= tol * scale, "%s: %.3e against float64 autograd (scale %.3e)" % (what, err, scale)


def _ncdhw(t):
  return t.permute(0, 4, 1, 2, 3)


# ----------------------------------------------------------------------------- (a)
def _torch_soft(l):
  D = l.shape[1]
  p = torch.softmax(l, 1)
  pred = (p * torch.arange(D, dtype=l.dtype).reshape(1, D, 1, 1)).sum(1)
  srt = torch.sort(l, 1, descending=True)[0]
  fcs = srt[:, 0] - srt[:, 2:].mean(1) if D > 2 else torch.zeros_like(pred)
  return pred, torch.argmax(l, 1), fcs


@pytest.mark.parametrize("geom", [(1, 1, 1, 32), (1, 2, 2, 31), (3, 3, 2, 17), (1, 9, 5, 9), (2, 32, 3, 17), (2, 12, 6, 19)], ids=tr.geom_id)
@pytest.mark.parametrize("affine", [0, 1])
def test_restatements_equal_float64_autograd(geom, affine):
  c = tr.fwd_case(geom, 5.0)
  b = tr.bwd_case(geom, 5.0)
  sc, sh = (c["scale"], c["shift"]) if affine else (None, None)
  ref = tr.forward(c["x"], c["w"], c["b"], sc, sh)
  x64 = c["x"].double()
  a64 = F.leaky_relu(x64 * sc.double() + sh.double(), tr.SLOPE) if affine else x64
  a64 = a64.clone().requires_grad_(True)
  w64, b64 = c["w"].double()[None].clone().requires_grad_(True), c["b"].double().clone().requires_grad_(True)
  logits = F.conv3d(_ncdhw(a64), w64, b64, padding=1)[:, 0]
  _close(ref["a"], a64.detach(), "operand")
  _close(ref["logits"], logits.detach(), "logits")
  # the soft-argmax stage and the backward from the SAME fp32 logits (the backward's input is what the forward saved)
  l32 = logits.detach().float()
  s = tr.soft_stage(l32)
  pred, am, fcs = _torch_soft(l32.double())
  _close(s["pred"], pred, "pred")
  _close(s["fcs"], fcs, "fcs")
  assert bool(torch.equal(s["argmax"], am))
  # autograd through soft-argmax(conv3d): logits replaced by their fp32 values via a straight-through offset
  off = (l32.double() - logits.detach())
  pred2 = _torch_soft(logits + off)[0]
  ((pred2 * b["g_pred"].double()).sum() + ((logits + off) * b["g_in"].double()).sum()).backward()
  got = tr.tail_backward(l32, a64.detach(), c["w"], b["g_pred"], b["g_in"])
  _close(got["g_a"], a64.grad, "g_a")
  _close(got["g_w"], w64.grad[0], "g_w")
  _close(got["g_b"], b64.grad, "g_bias")
  acc = tr.tail_backward(l32, a64.detach(), c["w"], b["g_pred"], b["g_in"], b["gw0"], b["gb0"])
  _close(acc["g_w"], w64.grad[0] + b["gw0"].double(), "accumulated g_w")
  _close(acc["g_b"], b64.grad + b["gb0"].double(), "accumulated g_bias")
  for k in ("e_logits", "e_pred", "e_fcs"):
    v = ref[k] if k in ref else s[k]
    assert bool((v >= 0).all()) and bool(torch.isfinite(v).all())


@pytest.mark.parametrize("geom", tr.CV_GEOMS + [(2, 5, 2, 7)], ids=tr.geom_id)
def test_cost_volume_restatement_equals_float64_autograd(geom):
  B, D, H, W = geom
  c = tr.cv_case(geom)
  L, R = c["L"].double().requires_grad_(True), c["R"].double().requires_grad_(True)
  vol = torch.zeros(B, D, H, W, 32, dtype=F64)
  for d in range(min(D, W)):                                   # the reference model's loop of slice assignments
    vol[:, d, :, d:] = (L[:, :, :, d:] - R[:, :, :, :W - d]).permute(0, 2, 3, 1)
  assert bool(torch.equal(tr.cost_volume(c["L"], c["R"], D), vol.detach().float()))
  vol.backward(c["gvol"].double())
  ref = tr.cost_volume_bwd(c["gvol"])
  _close(ref["gL"], L.grad, "gL")
  _close(ref["gR"], R.grad, "gR")
  # the number of terms per column: D = 64 > W = 17 gives x + 1 and W - x
  assert float(ref["nL"][0]) == 1 and float(ref["nL"][W - 1]) == min(W - 1, D - 1) + 1
  assert float(ref["nR"][W - 1]) == 1 and float(ref["nR"][0]) == min(W, D)


# ----------------------------------------------------------------------------- (b)
# the six cases of the soft-argmax margin, then the small geometries of the tables
SOFT_CASES = [((1, 8, 5, 9), 1.0), ((2, 12, 6, 19), 50.0), ((1, 24, 4, 33), 300.0), ((2, 12, 24, 78), 20.0), ((1, 32, 3, 17), 100.0),
              ((1, 3, 2, 40), 5.0)]
SMALL_FWD = [g for g, _ in tr.FWD_GEOMS if g[0] * g[1] * g[2] * g[3] <= 4000]
SMALL_BWD = [g for g, _ in tr.BWD_GEOMS if g[0] * g[1] * g[2] * g[3] <= 8000]


def test_fp32_emulations_stay_inside_every_bound(capsys):
  worst = {}

  def see(name, got, ref, bound):
    r = tr.ratio(got, ref, bound)
    worst[name] = max(worst.get(name, 0.0), r)
    assert r <= 1.0, "%s: err / bound %.3g" % (name, r)

  for geom, gain in SOFT_CASES + [(g, k) for g in SMALL_FWD for k in tr.GAINS]:
    c = tr.fwd_case(geom, gain)
    for affine in (0, 1):
      sc, sh = (c["scale"], c["shift"]) if affine else (None, None)
      ref = tr.forward(c["x"], c["w"], c["b"], sc, sh)
      a32 = c["x"] if not affine else F.leaky_relu(c["x"] * sc + sh, tr.SLOPE)
      if affine:
        see("operand (affine)", a32, ref["a"], ref["e_a"])
      l32 = tr.logits_sum(a32, c["w"], c["b"], torch.float32)
      see("logits: project and shift", l32, ref["logits"], ref["e_logits"])
      see("logits: torch fp32", F.conv3d(_ncdhw(a32), c["w"][None], c["b"], padding=1)[:, 0], ref["logits"], ref["e_logits"])
      s = tr.soft_stage(l32)
      e = tr.soft_sum(l32, torch.float32)
      see("pred", e["pred"], s["pred"], s["e_pred"])
      if geom[1] > 2:
        see("fcs", e["fcs"], s["fcs"], s["e_fcs"])
      else:
        assert float(e["fcs"].abs().max()) == 0.0 and float(s["e_fcs"].abs().max()) == 0.0
      assert bool(torch.equal(e["argmax"], s["argmax"]))
      ok = tr.decided(ref["logits"], ref["e_logits"])
      assert bool((e["argmax"][ok] == torch.argmax(ref["logits"], 1)[ok]).all())
  for geom in SMALL_BWD:
    for gain in tr.GAINS:
      b = tr.bwd_case(geom, gain)
      for gp, gi, acc in ((1, 1, 0), (1, 0, 1), (0, 1, 1)):
        kw = dict(g_pred=b["g_pred"] if gp else None, g_in=b["g_in"] if gi else None, gw0=b["gw0"] if acc else None,
                  gb0=b["gb0"] if acc else None)
        ref = tr.tail_backward(b["logits"], b["a"], b["w"], **kw)
        e = tr.tail_backward(b["logits"], b["a"], b["w"], dtype=torch.float32, **kw)
        see("g_logits", e["gl"], ref["gl"], ref["e_gl"])
        see("g_a", e["g_a"], ref["g_a"], ref["e_g_a"])
        see("g_w", e["g_w"], ref["g_w"], ref["e_g_w"])
        see("g_bias", e["g_b"], ref["g_b"], ref["e_g_b"])
  for geom in tr.CV_GEOMS:
    c = tr.cv_case(geom)
    ref = tr.cost_volume_bwd(c["gvol"])
    e = tr.cost_volume_bwd(c["gvol"], torch.float32)
    see("cost volume gL", e["gL"], ref["gL"], ref["e_gL"])
    see("cost volume gR", e["gR"], ref["gR"], ref["e_gR"])
  with capsys.disabled():
    for k in sorted(worst):
      print("  tail_ref bracketing: worst err / bound %-28s %.4f" % (k, worst[k]))


def test_crafted_families_are_exact_in_fp32():
  """single tap: each logit is a shifted copy plus the bias, zero across the borders; backward: g_a a shifted copy scaled by a
  power of two, g_w sums of two exact products, g_bias an integer sum — the float64 value IS an fp32 number and the fp32
  emulation gives it bit for bit"""
  for geom in [(3, 3, 2, 17), (1, 1, 1, 32)]:
    B, D, H, W = geom
    for t, (kd, kh, kw) in enumerate(tr.TAPS):
      c = tr.tap_case(geom, t)
      z = tr.logits_sum(c["x"], c["w"], c["b"])
      assert bool(torch.equal(z.float().double(), z)) and bool(torch.equal(tr.logits_sum(c["x"], c["w"], c["b"], torch.float32).double(), z))
      ch = F.pad(c["x"][..., (5 * t + 3) % 32].double(), (1, 1, 1, 1, 1, 1))
      assert bool(torch.equal(z, ch[:, kd:kd + D, kh:kh + H, kw:kw + W] + float(c["b"])))
  for geom in [(2, 2, 3, 13), (1, 12, 4, 14), (1, 3, 1, 1)]:
    for t in range(27):
      for spot in tr.BWD_SPOTS:
        c = tr.bwd_exact_case(geom, t, spot)
        for acc in (0, 1):
          r = tr.tail_backward(c["logits"], c["a"], c["w"], None, c["g_in"], c["gw0"] if acc else None, c["gb0"] if acc else None)
          e = tr.tail_backward(c["logits"], c["a"], c["w"], None, c["g_in"], c["gw0"] if acc else None, c["gb0"] if acc else None,
                               dtype=torch.float32)
          assert bool(torch.equal(r["gl"], c["g_in"].double())) and float(r["e_gl"].abs().max()) == 0.0
          for k in ("g_a", "g_w", "g_b"):
            assert bool(torch.equal(r[k].float().double(), r[k])) and bool(torch.equal(e[k].double(), r[k])), (geom, t, spot, k)


def test_designed_logits_hold_the_ties_they_name():
  c = tr.designed_case((2, 32, 3, 17), 16)
  assert bool(torch.equal(tr.logits_sum(c["x"], c["w"]), c["l"].double()))
  s = tr.soft_sum(c["l"])
  at = lambda name, tag: tuple(c["where"][(name, tag)])
  for tag in ("first", "last", "tile"):
    b, y, x = at("three-way tie", tag)
    assert int(s["argmax"][b, y, x]) == 1
    b, y, x = at("tie d, d + 8 (one lane)", tag)
    assert int(s["argmax"][b, y, x]) == 1
    b, y, x = at("all equal", tag)
    assert int(s["argmax"][b, y, x]) == 0 and float(s["fcs"][b, y, x]) == 0.0
    b, y, x = at("maximum at D - 1", tag)
    assert int(s["argmax"][b, y, x]) == 31
    b, y, x = at("duplicate maximum", tag)
    assert float(s["fcs"][b, y, x]) == 4.0 - 1.0 / 30.0
    b, y, x = at("+-3e4", tag)
    assert float(s["pred"][b, y, x]) == 0.0 and bool(torch.isfinite(s["fcs"][b, y, x]))
  # the tile spot lies inside the last tile's overlap with its neighbour: positions [npos - 16, 16 * (tiles - 1))
  H, W = 3, 17
  n = tr.fwd_npos(H, W)
  b, y, x = at("all equal", "tile")
  assert n - 16 <= y * (W + 2) + x < n


# ----------------------------------------------------------------------------- (c)
MUT_FWD = [(1, 2, 2, 31), (3, 3, 2, 17), (1, 9, 5, 9), (2, 32, 3, 17)]
MUT_BWD = [(2, 2, 3, 13), (1, 12, 4, 14), (2, 32, 3, 27), (1, 3, 769, 3)]


def _caught_logits(mut):
  hits = []
  for geom in MUT_FWD:
    m = (mut[0], tr.fwd_route(geom)) if mut is not None and mut[0] == "no_shift_back" else mut
    for fam in ["random"] + [("tap", t) for t in range(27)]:
      c = tr.fwd_case(geom) if fam == "random" else tr.tap_case(geom, fam[1])
      ref = tr.forward(c["x"], c["w"], c["b"])
      got = tr.logits_sum(c["x"], c["w"], c["b"], mut=m)
      bad = tr.ratio(got, ref["logits"], ref["e_logits"]) > 1.0 if fam == "random" else not bool(torch.equal(got, ref["logits"]))
      if bad:
        hits.append((geom, fam))
  return hits


def _caught_soft(mut):
  hits = []
  for geom in MUT_FWD:
    cases = [("random %g" % k, tr.forward(**{n: v for n, v in tr.fwd_case(geom, k).items() if n in ("x", "w")})["logits"].float())
             for k in tr.GAINS]
    cases.append(("designed", tr.designed_case(geom, tr.fwd_route(geom))["l"]))
    for name, l in cases:
      s = tr.soft_stage(l)
      got = tr.soft_sum(l, mut=mut)
      bad = tr.ratio(got["pred"], s["pred"], s["e_pred"]) > 1.0 or tr.ratio(got["fcs"], s["fcs"], s["e_fcs"]) > 1.0 or \
          not bool(torch.equal(got["argmax"], s["argmax"]))
      if bad:
        hits.append((geom, name))
  return hits


def _caught_bwd(mut):
  hits = []
  for geom in MUT_BWD:
    xc = tr.bwd_route(geom)
    fams = ["random"] + [("exact", t, s) for t in (0, 4, 13, 22, 26) for s in tr.BWD_SPOTS]
    for fam in fams:
      c = tr.bwd_case(geom, 50.0) if fam == "random" else tr.bwd_exact_case(geom, fam[1], fam[2], xc)
      ref = tr.tail_backward(c["logits"], c["a"], c["w"], c["g_pred"], c["g_in"])
      got = tr.tail_backward(c["logits"], c["a"], c["w"], c["g_pred"], c["g_in"], mut=mut, xc=xc)
      if fam == "random":
        bad = any(tr.ratio(got[k], ref[k], ref["e_" + k]) > 1.0 for k in ("g_a", "g_w", "g_b"))
      else:
        bad = not all(bool(torch.equal(got[k], ref[k])) for k in ("g_a", "g_w", "g_b"))
      if bad:
        hits.append((geom, fam))
  return hits


CAUGHT = {"logits": _caught_logits, "soft": _caught_soft, "bwd": _caught_bwd}


@pytest.mark.parametrize("name", sorted(tr.MUTANTS))
def test_every_wrong_restatement_is_caught(name, capsys):
  stage, mut = tr.MUTANTS[name]
  hits = CAUGHT[stage](mut)
  with capsys.disabled():
    print("  tail_ref mutant '%s': caught in %d cases, first %s" % (name, len(hits), hits[:1]))
  assert hits, "no case tells '%s' from the right restatement" % name


def test_the_right_restatement_is_not_caught():
  assert _caught_logits(None) == [] and _caught_soft(None) == [] and _caught_bwd(None) == []


# ----------------------------------------------------------------------------- (d)
def test_every_route_follows_from_the_tables_arithmetic():
  for geom, n in tr.FWD_GEOMS:
    B, D, H, W = geom
    tiles32 = B * ((tr.fwd_npos(H, W) + 31) // 32)
    assert tr.fwd_route(geom) == n == (16 if tiles32 < 512 else 32), (geom, tiles32)
    assert B * (D + 2) * (H + 2) * (W + 2) * 128 < 70e6
  tiles = {g: g[0] * ((tr.fwd_npos(g[2], g[3]) + 31) // 32) for g, _ in tr.FWD_GEOMS}
  assert tiles[(8, 12, 24, 78)] == 480 and tiles[(511, 3, 1, 32)] == 511 and tiles[(512, 3, 1, 32)] == 512
  assert tiles[(171, 5, 2, 40)] == 513 and tiles[(9, 12, 24, 78)] == 540 and tiles[(13, 4, 8, 156)] == 520
  assert tr.fwd_npos(1, 32) == 32 and tr.fwd_grid((1, 1, 1, 32)) == 2 and tr.fwd_grid((3, 3, 2, 17)) == 9
  assert tr.fwd_npos(2, 17) % 16 != 0 and tr.fwd_npos(2, 40) % 32 != 0 and tr.fwd_npos(5, 9) % 16 != 0      # shifted-back last tiles
  assert tr.fwd_grid((171, 5, 2, 40)) % 8 == 1
  assert [tr.fwd_route(g) for g in tr.FWD_REFUSED] == [0, 0, 0] and tr.fwd_route((1, 12, 3, 173)) == 16
  assert tr.fwd_npos(1, 31) == 31
  for geom, xc in tr.BWD_GEOMS:
    B, D, H, W = geom
    assert tr.bwd_route(geom) == xc == (26 if B * H * ((W + 25) // 26) > 768 else 13), geom
    assert B * (D + 2) * (H + 2) * (W + 2) * 128 < 70e6
  assert 32 * 24 * 1 == 768 and tr.bwd_units((32, 3, 24, 26)) == 1536 and tr.bwd_units((32, 3, 24, 27)) == 1536
  assert tr.bwd_units((1, 3, 769, 3)) == 769 and tr.bwd_units((11, 12, 24, 78)) == 792
  for g in tr.FWD_ONCE | set(tr.FWD_TAP_GEOMS) | set(tr.FWD_DESIGNED_GEOMS):
    assert tr.fwd_route(g) in (16, 32)
  assert {tr.fwd_route(g) for g in tr.FWD_ONCE} == {16, 32} == {tr.fwd_route(g) for g in tr.FWD_DESIGNED_GEOMS}
  assert {tr.bwd_route(g) for g in tr.BWD_EXACT_GEOMS} == {13, 26}


@pytest.mark.parametrize("geom", [g for g, _ in tr.FWD_GEOMS], ids=tr.geom_id)
def test_the_undecided_share_stays_below_the_cap(geom, capsys):
  worst = 0.0
  for gain in tr.GAINS:
    c = tr.fwd_case(geom, gain)
    for affine in (0, 1):
      ref = tr.forward(c["x"], c["w"], c["b"], *((c["scale"], c["shift"]) if affine else (None, None)))
      ok = tr.decided(ref["logits"], ref["e_logits"])
      share = 1.0 - float(ok.double().mean())
      worst = max(worst, share)
      assert share < tr.UNDECIDED_CAP, "%s gain %g affine %d: %.2f %% of the pixels undecided" % (geom, gain, affine, 100 * share)
  with capsys.disabled():
    print("  tail_ref undecided arg-max share %-14s at most %.3f %%" % (tr.geom_id(geom), 100 * worst))
