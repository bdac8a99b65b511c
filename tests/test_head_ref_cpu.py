"""tests/head_ref.py on the CPU: (a) the float64 restatements of the feature head's 5x5 stride-2 launches against float64 autograd
of F.conv2d; (b) two fp32 emulations of each launch — torch's own fp32 convolution and a tap-by-tap fp32 accumulation in the
kernels' tap order — inside every derived bound on every generator case, the worst err / bound printed; (c) the cases
discriminate: every deliberately wrong restatement of head_ref.MUTANTS exceeds a bound, breaks bit-exactness or touches the
halo in at least one case of the smallest geometries.  (c) is what keeps tests/test_gpu_head_fp64.py from passing vacuously."""
import pytest
import torch
import torch.nn.functional as F

import head_ref as hr


def _nchw(t):
  return t.permute(0, 3, 1, 2)


def _autograd64(x, w, b, gz):
  x64 = _nchw(x.double()).clone().requires_grad_(True)
  w64, b64 = w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
  z = F.conv2d(x64, w64, b64, stride=2, padding=2)
  z.backward(_nchw(gz.double()))
  return z.detach().permute(0, 2, 3, 1), x64.grad.permute(0, 2, 3, 1), w64.grad, b64.grad


def _close(a, b, what):
  scale = max(float(b.abs().max()), 1.0)
  err = float((a - b).abs().max())
  assert err <= 1e-12 * scale, "%s: %.3e against float64 autograd (scale %.3e)" % (what, err, scale)


# ----------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("geom,cin", [((1, 1, 1), 32), ((2, 2, 2), 32), ((1, 5, 7), 32), ((2, 9, 13), 3), ((2, 6, 12), 32),
                                      ((1, 7, 66), 32), ((1, 8, 67), 3)], ids=lambda v: str(v))
def test_restatements_equal_float64_autograd(geom, cin):
  B, H, W = geom
  c = hr.fwd_case(geom, "random", cin)
  Ho, Wo = hr.out_extent(H), hr.out_extent(W)
  gz = torch.randn(B, Ho, Wo, 32, generator=torch.Generator().manual_seed(9))
  z, gx, dW, db = _autograd64(c["x"], c["w"], c["b"], gz)
  _close(hr.forward(c["x"], c["w"], c["b"])["z"], z, "forward")
  got_dW, got_db = hr.wgrad_sum(c["x"], gz)
  _close(got_dW, dW, "weight gradient")
  _close(got_db, db, "bias gradient")
  if cin == 32:
    for pz in (1, 2):
      g = hr.data_gradient(gz, c["w"], H, W, pz=pz)["g_x"]
      assert hr.halo_kept(g)
      _close(g[:, 1:-1, 1:-1], gx, "data gradient")
    d0, b0 = torch.randn(32, cin, 5, 5), torch.randn(32)
    acc = hr.weight_gradient(c["x"], gz, d0, b0)
    _close(acc["dW"], dW + d0.double(), "accumulated weight gradient")
    _close(acc["db"], db + b0.double(), "accumulated bias gradient")


def test_phase_terms_are_9_6_6_4_taps():
  n = hr.phase_terms(4, 5)
  assert n[0, 0] == 288 and n[0, 1] == 192 and n[1, 0] == 192 and n[1, 1] == 128 and n[2, 4] == 288 and n[3, 3] == 128
  assert [len(hr.phase_taps(py, px)) for (py, px) in hr.PHASES] == [9, 6, 6, 4]
  assert sorted(t for ph in hr.PHASES for t in hr.phase_taps(*ph)) == hr.TAPS


def test_segment_steps_of_the_issue_geometries():
  # 47 x 156 in 3 segments: 32 / 32 / 14 pair-steps; 66 wide in 2: 24 + 9; 67 wide in 2: 24 + 10
  assert hr.seg_steps(156, 3) == 32 and hr.seg_steps(66, 2) == 24 and hr.seg_steps(67, 2) == 24 and hr.seg_steps(7, 1) == 8


# ----------------------------------------------------------------------------- (b)
# the generator cases at extents the CPU convolves in a moment: every parity class, a ragged segment, more than one segment
BRACKET_GEOMS = [(1, 1, 1), (1, 2, 2), (1, 5, 7), (2, 9, 13), (2, 6, 12), (1, 5, 131), (2, 7, 133), (3, 21, 33), (2, 15, 66)]


def _fwd32(c):
  return F.conv2d(_nchw(c["x"]), c["w"], c["b"], stride=2, padding=2).permute(0, 2, 3, 1)


def test_fp32_emulations_stay_inside_every_bound(capsys):
  worst = {}

  def see(name, got, ref, bound):
    r = hr.ratio(got, ref, bound)
    worst[name] = max(worst.get(name, 0.0), r)
    assert r <= 1.0, "%s: err / bound %.3g" % (name, r)

  for geom in BRACKET_GEOMS:
    B, H, W = geom
    for cin in (3, 32):
      c = hr.fwd_case(geom, "random", cin)
      ref = hr.forward(c["x"], c["w"], c["b"])
      see("forward cin %d: torch fp32" % cin, _fwd32(c), ref["z"], ref["e_z"])
      see("forward cin %d: tap by tap" % cin, hr.fwd_sum(c["x"], c["w"], c["b"], torch.float32), ref["z"], ref["e_z"])
      for nseg in (1, 2):
        w = hr.wgrad_case(geom, "random", cin, nseg)
        ref = hr.weight_gradient(w["x"], w["gz"])
        x32 = _nchw(w["x"]).clone().requires_grad_(True)
        w32, b32 = torch.zeros(32, cin, 5, 5, requires_grad=True), torch.zeros(32, requires_grad=True)
        F.conv2d(x32, w32, b32, stride=2, padding=2).backward(_nchw(w["gz"]))
        see("dW cin %d: torch fp32" % cin, w32.grad, ref["dW"], ref["e_dW"])
        see("db cin %d: torch fp32" % cin, b32.grad, ref["db"], ref["e_db"])
        dW32, db32 = hr.wgrad_sum(w["x"], w["gz"], torch.float32)
        see("dW cin %d: tap by tap" % cin, dW32, ref["dW"], ref["e_dW"])
        see("db cin %d: tap by tap" % cin, db32, ref["db"], ref["e_db"])
    d = hr.dgrad_case(geom, "random")
    ref = hr.data_gradient(d["gz"], d["w"], H, W)
    x32 = torch.zeros(B, 32, H, W, requires_grad=True)
    F.conv2d(x32, d["w"], None, stride=2, padding=2).backward(_nchw(d["gz"]))
    see("data gradient: torch fp32", x32.grad.permute(0, 2, 3, 1), ref["g_x"][:, 1:-1, 1:-1], ref["e_g_x"])
    see("data gradient: tap by tap", hr.dgrad_sum(d["gz"], d["w"], H, W, torch.float32)[:, 1:-1, 1:-1], ref["g_x"][:, 1:-1, 1:-1],
        ref["e_g_x"])
  with capsys.disabled():
    for k in sorted(worst):
      print("  head_ref bracketing: worst err / bound %-34s %.4f" % (k, worst[k]))


def test_crafted_families_are_exact_in_fp32():
  """single tap: forward and data gradient are copies scaled by a power of two; two impulses: every dW entry is a sum of two
  exactly representable products — the float64 value IS an fp32 number and the fp32 emulation gives it bit for bit"""
  for geom in [(1, 5, 7), (2, 6, 12), (1, 5, 131)]:
    B, H, W = geom
    for t in range(25):
      for cin in (3, 32):
        c = hr.fwd_case(geom, ("tap", t), cin)
        z = hr.fwd_sum(c["x"], c["w"], c["b"])
        assert bool(torch.equal(z.float().double(), z)) and bool(torch.equal(hr.fwd_sum(c["x"], c["w"], c["b"], torch.float32).double(), z))
      d = hr.dgrad_case(geom, ("tap", t))
      g = hr.dgrad_sum(d["gz"], d["w"], H, W)[:, 1:-1, 1:-1]
      assert bool(torch.equal(g.float().double(), g))
      assert bool(torch.equal(hr.dgrad_sum(d["gz"], d["w"], H, W, torch.float32)[:, 1:-1, 1:-1].double(), g))
    for spot in hr.IMPULSE_SPOTS:
      for nseg in (1, 2):
        w = hr.wgrad_case(geom, ("impulse", spot), 32, nseg)
        dW, db = hr.wgrad_sum(w["x"], w["gz"])
        assert bool(torch.equal(dW.float().double(), dW)) and bool(torch.equal(db.float().double(), db))
        assert bool(torch.equal(hr.wgrad_sum(w["x"], w["gz"], torch.float32)[0].double(), dW))
        assert float(dW.abs().max()) > 0


# ----------------------------------------------------------------------------- (c)
# the smallest geometries of the GPU file's routes (a mutant needs an odd H, an odd Wo or two segments to exist at all)
SMALL_FWD = [(1, 9, 13), (3, 21, 33), (2, 6, 12)]
SMALL_DGRAD = [(1, 1, 1), (1, 2, 2), (1, 5, 7), (2, 6, 12)]
SMALL_WGRAD = [((1, 9, 13), 1), ((1, 5, 131), 2), ((2, 7, 133), 2)]


def _caught_fwd(mut):
  hits = []
  for geom in SMALL_FWD:
    for fam in ["random"] + [("tap", t) for t in range(25)]:
      c = hr.fwd_case(geom, fam)
      ref = hr.forward(c["x"], c["w"], c["b"])
      got = hr.fwd_sum(c["x"], c["w"], c["b"], mut=mut)
      bad = (not bool(torch.equal(got, ref["z"]))) if fam != "random" else hr.ratio(got, ref["z"], ref["e_z"]) > 1.0
      if bad:
        hits.append((geom, fam))
  return hits


def _caught_dgrad(mut, pz=1):
  hits = []
  for geom in SMALL_DGRAD:
    B, H, W = geom
    for fam in ["random"] + [("tap", t) for t in range(25)]:
      d = hr.dgrad_case(geom, fam)
      ref = hr.data_gradient(d["gz"], d["w"], H, W, pz=pz)
      got = hr.dgrad_sum(d["gz"], d["w"], H, W, pz=pz, mut=mut)
      gi, ri = got[:, 1:-1, 1:-1], ref["g_x"][:, 1:-1, 1:-1]
      bad = not hr.halo_kept(got)
      bad = bad or ((not bool(torch.equal(gi, ri))) if fam != "random" else hr.ratio(gi, ri, ref["e_g_x"]) > 1.0)
      if bad:
        hits.append((geom, fam))
  return hits


def _caught_wgrad(mut):
  hits = []
  for geom, nseg in SMALL_WGRAD:
    for fam in ["random"] + [("impulse", s) for s in hr.IMPULSE_SPOTS]:
      w = hr.wgrad_case(geom, fam, 32, nseg)
      ref = hr.weight_gradient(w["x"], w["gz"])
      dW, db = hr.wgrad_sum(w["x"], w["gz"], mut=mut, nseg=nseg)
      if fam == "random":
        bad = hr.ratio(dW, ref["dW"], ref["e_dW"]) > 1.0 or hr.ratio(db, ref["db"], ref["e_db"]) > 1.0
      else:
        bad = not (bool(torch.equal(dW, ref["dW"])) and bool(torch.equal(db, ref["db"])))
      if bad:
        hits.append((geom, fam))
  return hits


@pytest.mark.parametrize("name", sorted(hr.MUTANTS))
def test_every_wrong_restatement_is_caught(name, capsys):
  op, mut = hr.MUTANTS[name]
  hits = {"fwd": _caught_fwd, "dgrad": _caught_dgrad, "wgrad": _caught_wgrad}[op](mut)
  with capsys.disabled():
    print("  head_ref mutant '%s': caught in %d cases, first %s" % (name, len(hits), hits[:1]))
  assert hits, "no case tells '%s' from the right restatement" % name


def test_the_right_restatement_is_not_caught():
  assert _caught_fwd(None) == [] and _caught_dgrad(None) == [] and _caught_dgrad(None, pz=2) == [] and _caught_wgrad(None) == []


def test_an_early_clamp_inside_a_zero_halo_of_two_changes_no_value():
  """The forward kernels' right-edge clamp lands on the LAST padded column; one voxel early it lands on the other halo column
  of the input's halo of 2, which holds zero as well — and so does the data gradient's with a g_z halo of 2.  No value can
  tell: only the data gradient with a g_z halo of 1 (clamped into the last interior column) is caught above."""
  assert _caught_fwd(("clamp_early", 1)) == []
  assert _caught_dgrad(("clamp_early", 1), pz=2) == []
  assert _caught_dgrad(("clamp_early", 1), pz=1) != []
