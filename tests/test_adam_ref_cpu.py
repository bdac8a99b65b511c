"""tests/adam_ref.py held to torch on the CPU: the double-hyper-parameter form is torch.optim.Adam + clip_grad_norm_ in float64 to
float64 noise over several steps, and the float32-hyper-parameter form (what the C ABI receives) stays at the derived distance
from it: ``rel_1m(b2)`` on the new term of exp_avg_sq, at most half of that (plus the float32 roundings of lr and b1) on the
update."""
import math

import torch

import adam_ref as ar

LR, B1, B2, EPS, MAX_NORM = 5e-5, 0.9, 0.999, 1e-8, 1.0


def _rnd(n, seed, scale=1.0):
  return (torch.rand(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1) * scale


def test_double_form_is_torch_adam_with_clip_in_float64():
  """7 steps, two parameter tensors (the clip norm is global), gradient norms below and above max_norm"""
  shapes = [(37,), (5, 11)]
  params = [torch.nn.Parameter(_rnd(math.prod(s), 1 + i).reshape(s)) for i, s in enumerate(shapes)]
  opt = torch.optim.Adam(params, lr=LR, betas=(B1, B2), eps=EPS)
  hp = ar.hyper(LR, B1, B2, EPS, False)
  p = torch.cat([q.detach().reshape(-1) for q in params]).clone()
  m, v = torch.zeros_like(p), torch.zeros_like(p)
  clipped = []
  for t in range(1, 8):
    g = _rnd(p.numel(), 10 + t, scale=[1e-3, 0.5, 2.0, 1e-2, 1.0, 0.05, 30.0][t - 1])
    off = 0
    for q in params:
      q.grad = g[off:off + q.numel()].reshape(q.shape).clone(); off += q.numel()
    torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
    opt.step()
    coef = ar.clip_coef(float((g * g).sum()), MAX_NORM)
    clipped.append(coef < 1.0)
    out = ar.step(p, g * coef, m, v, t, hp)
    p, m, v = out["p"], out["m"], out["v"]
    got_p = torch.cat([q.detach().reshape(-1) for q in params])
    got_m = torch.cat([opt.state[q]["exp_avg"].reshape(-1) for q in params])
    got_v = torch.cat([opt.state[q]["exp_avg_sq"].reshape(-1) for q in params])
    # float64 noise of a few steps, relative to the largest entry (an exp_avg that cancels has no relative accuracy of its own)
    assert float((got_m - m).abs().max()) <= 1e-14 * float(m.abs().max()), t
    assert float((got_v - v).abs().max()) <= 1e-14 * float(v.abs().max()), t
    assert float((got_p - p).abs().max()) <= 1e-15, t           # |p| ~ 1: a few ulp of float64
  assert any(clipped) and not all(clipped)


def test_distance_between_float32_and_double_hyper_parameters():
  rel = ar.rel_1m(B2)
  b2f = ar.f32(B2)
  assert rel == abs(B2 - b2f) / (1.0 - B2)                       # 1 - b is exact: the difference is the rounding of b itself
  assert 1.28e-5 < rel < 1.30e-5                                 # 0.999 -> 0x3F7FBE77: 1.29e-5
  hd, hf = ar.hyper(LR, B1, B2, EPS, False), ar.hyper(LR, B1, B2, EPS, True)
  n = 4096
  g, m0, v0 = _rnd(n, 1, 1e-2), _rnd(n, 2, 1e-3), _rnd(n, 3, 1e-5).abs() + 1e-8
  # the new term of exp_avg_sq, alone (v = 0): exactly rel, up to float64 noise
  vd = ar.moments(g, torch.zeros(n), torch.zeros(n), hd)[1]
  vf = ar.moments(g, torch.zeros(n), torch.zeros(n), hf)[1]
  assert float(((vf / vd - 1.0).abs() - rel).abs().max()) <= 1e-12
  # the update: half of rel from sqrt(v' / bc2) (both move the same way with b2), the float32 roundings of lr and eps (2^-24
  # each) and of b1 in (1 - b1) and in bc1 (|b1 - b1_f32| / (1 - b1) each)
  allow = 0.5 * rel + 2 * ar.U + 2 * ar.rel_1m(B1)
  worst = 0.0
  for t in (1, 2, 3, 10, 1000, 100000, 2 ** 24 - 1):
    for m, v in ((torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)), (m0, v0)):
      ud = ar.step(torch.zeros(n), g, m, v, t, hd)["update"]
      uf = ar.step(torch.zeros(n), g, m, v, t, hf)["update"]
      # (where m' cancels, the rounding of b1 is relative to m's terms, not to m')
      terms = ar.moments(g, m, v, hd)[2] / ar.moments(g, m, v, hd)[0].abs()
      ratio = float(((uf - ud).abs() / (ud.abs() * (0.5 * rel + 2 * ar.U + 2 * ar.rel_1m(B1) * terms))).max())
      worst = max(worst, ratio)
  print("update: float32- vs double-hyper-parameter form at %.3f of %.3e" % (worst, allow))
  assert worst <= 1.0
  assert worst >= 0.3            # and the deviation is really there: the bound is not slack by an order of magnitude


def test_clip_coefficient_forms_agree():
  for s in (0.0, 1e-12, 0.25, 1.0, 1.0000001, 4.0, 1e6):
    c32 = float(ar.clip_coef32(torch.tensor(s, dtype=torch.float32), MAX_NORM))
    c64 = ar.clip_coef(ar.f32(s), MAX_NORM)
    assert abs(c32 - c64) <= 3 * ar.U * c64, (s, c32, c64)
  assert float(ar.clip_coef32(torch.tensor(0.0), MAX_NORM)) == 1.0
