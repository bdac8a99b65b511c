"""The fp64 BatchNorm reference (bn_ref.py) and its error models, on the CPU: the GPU BatchNorm tests are only as good as
they are."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref as br


def _data(N, C, seed, offset=0.0):
  g = torch.Generator().manual_seed(seed)
  return (torch.randn(N, C, generator=g, dtype=torch.float64) * (1 + torch.arange(C, dtype=torch.float64)) + offset)


@pytest.mark.parametrize("N,offset", [(1, 0.0), (2, 3.0), (97, 0.0), (1000, 1e3)])
def test_reference_is_torch_batch_norm_in_float64(N, offset):
  """forward state, running statistics (the count-1 fallback included) and all three gradients against F.batch_norm and its
  autograd in float64"""
  C = 5
  z = _data(N, C, seed=N, offset=offset).requires_grad_(True)
  g = torch.Generator().manual_seed(7)
  gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
  beta = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_(True)
  rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
  rm_t, rv_t = rm.clone(), rv.clone()
  if N == 1:       # torch refuses a single value per channel in training mode: the fallback is the biased variance, 0
    st = br.bn_state64(*br.moments64(z.detach()), gamma.detach(), beta.detach(), rm, rv)
    assert torch.equal(st["var_u"], torch.zeros(C, dtype=torch.float64))
    assert torch.allclose(st["running_var"], 0.9 * rv, rtol=1e-15) and torch.equal(st["invstd"], torch.full((C,), br.EPS ** -0.5, dtype=torch.float64))
    return
  y = F.batch_norm(z.t().unsqueeze(0), rm_t, rv_t, gamma, beta, True, br.MOMENTUM, br.EPS)[0].t()
  cnt, mean, m2 = br.moments64(z.detach())
  st = br.bn_state64(cnt, mean, m2, gamma.detach(), beta.detach(), rm, rv)
  assert torch.allclose(z.detach() * st["scale"] + st["shift"], y.detach(), rtol=1e-12, atol=1e-12)
  assert torch.allclose(st["running_mean"], rm_t, rtol=1e-13, atol=1e-15)
  assert torch.allclose(st["running_var"], rv_t, rtol=1e-13, atol=1e-15)
  # the LeakyReLU on top, and its backward
  a = F.leaky_relu(y, br.SLOPE)
  g_a = torch.randn(N, C, generator=g, dtype=torch.float64) + 0.5
  a.backward(g_a)
  ref = br.bn_bwd64(g_a, z.detach(), dict(mean=mean, invstd=st["invstd"], scale=st["scale"], shift=st["shift"]), gamma.detach())
  if ref["n_amb"] == 0:
    for got, exp in ((ref["g_z"], z.grad), (ref["g_gamma"], gamma.grad), (ref["g_beta"], beta.grad)):
      assert torch.allclose(got, exp, rtol=1e-9, atol=1e-12 * float(exp.abs().max() + 1)), (got - exp).abs().max()


@pytest.mark.parametrize("splits", [[1], [7, 0, 3], [0, 0, 5, 1, 9], [1, 1, 1], [50, 0], [0, 1], [13, 1, 0, 86]])
def test_chan_merge_of_any_split_is_the_whole(splits):
  """any split into partials, empty ones (first, middle, last) and single-element ones included, merges to the moments of the
  whole to ~1e-15 relative"""
  C = 4
  N = sum(splits)
  z = _data(N, C, seed=N, offset=1e2)
  cnt, mean, m2, at = [], [], [], 0
  for n in splits:
    part = z[at:at + n]
    at += n
    cnt.append(float(n))
    if n:
      _, mu, q = br.moments64(part)
    else:
      mu, q = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    mean.append(mu); m2.append(q)
  n_all, mu_all, q_all = br.moments64(z)
  n_m, mu_m, q_m = br.chan_merge64(torch.tensor(cnt, dtype=torch.float64), torch.stack(mean), torch.stack(m2))
  assert n_m == n_all
  assert bool(((mu_m - mu_all).abs() <= 4e-15 * mu_all.abs().clamp(min=1)).all())
  assert bool(((q_m - q_all).abs() <= 4e-15 * q_all.abs() + 1e-300).all())


def test_chan_merge_ignores_what_an_empty_partial_holds():
  cnt = torch.tensor([0.0, 3.0, 0.0, 2.0], dtype=torch.float64)
  mean = torch.tensor([[float("nan")], [1.0], [1e30], [2.0]], dtype=torch.float64)
  m2 = torch.tensor([[float("inf")], [0.5], [-7.0], [0.25]], dtype=torch.float64)
  n, mu, q = br.chan_merge64(cnt, mean, m2)
  assert n == 5.0 and abs(float(mu) - 1.4) < 1e-15 and abs(float(q) - (0.75 + 3 * 0.16 + 2 * 0.36)) < 1e-14


def test_moments_per_group():
  z = _data(24, 3, seed=1, offset=5.0)
  cnt, mean, m2 = br.moments64(z, groups=2)
  for gi in range(2):
    c1, m1, q1 = br.moments64(z[12 * gi:12 * gi + 12])
    assert float(cnt[gi]) == c1 and torch.allclose(mean[gi], m1, rtol=1e-15) and torch.allclose(m2[gi], q1, rtol=1e-14)


def test_ulp32():
  x = torch.tensor([1.0, 1.5, 2.0, -3.0, 1e-3, 0.0], dtype=torch.float64)
  exp = [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -22, 2.0 ** -33, 2.0 ** -149]
  got = br.ulp32(x)
  for i in range(5):
    assert float(got[i]) == exp[i]
  assert float(got[5]) <= 2.0 ** -140


def test_merge_bounds_cover_a_one_pass_fp32_rounded_merge():
  """merge_bounds against an emulation of the kernels' one-pass pivot merge (fp64 sums, one rounding to fp32): the emulation
  stays within the bound, also with the pivot 1e5 standard deviations from the mean; and the bound stays under 1e-6 relative
  on invstd where the pivot is near the mean, so a merge that loses a partial fails it."""
  C, P = 3, 257
  g = torch.Generator().manual_seed(3)
  for far, offset in ((False, 1e4), (True, 1e5)):
    cnt = torch.randint(1, 4000, (P,), generator=g).double()
    mean = (torch.randn(P, C, generator=g, dtype=torch.float64) * 0.01 + offset).float().double()
    m2 = (torch.rand(P, C, generator=g, dtype=torch.float64) * cnt[:, None]).float().double()
    if far:
      mean[0] = mean[0] * 0 + offset * 2
    gamma, beta = torch.ones(C), torch.zeros(C)
    rm, rv = torch.zeros(C), torch.ones(C)
    n, mu, q = br.chan_merge64(cnt, mean, m2)
    st = br.bn_state64(n, mu, q, gamma, beta, rm, rv)
    K = mean[0]
    s0, s1, s2 = cnt.sum(), (cnt[:, None] * (mean - K)).sum(0), (m2 + cnt[:, None] * (mean - K) ** 2).sum(0)
    emu_mean = (K + s1 / s0).float().double()
    emu_var = (s2 - s1 * s1 / s0).clamp(min=0) / s0
    emu_inv = (1.0 / torch.sqrt(emu_var + br.EPS)).float().double()
    b = br.merge_bounds(cnt, mean, m2, gamma, st, c=P)
    assert bool(((emu_mean - st["mean"]).abs() <= b["mean"]).all())
    assert bool(((emu_inv - st["invstd"]).abs() <= b["invstd"]).all())
    if not far:
      assert bool((b["invstd"] <= 1e-6 * st["invstd"]).all())
      n2, mu2, q2 = br.chan_merge64(cnt[1:], mean[1:], m2[1:])
      inv2 = 1.0 / torch.sqrt(q2 / n2 + br.EPS)
      assert bool(((inv2 - st["invstd"]).abs() > 10 * b["invstd"]).any())


@pytest.mark.parametrize("n_lane,pivot_far", [(16, False), (300, False), (300, True), (4000, False)])
def test_producer_scales_cover_an_fp32_shifted_lane_sum(n_lane, pivot_far):
  """producer_scales against an fp32 emulation of the producers' lane sums (first element as the pivot, sequential fp32 adds
  and fmas, one fp32 Chan fold of 8 lanes per partial): the worst error stays within K = 16 of its scale, and the scale is
  tight enough that one dropped element of 1e4 standard deviations exceeds the bound by 10x at n_l = 16."""
  C, lanes = 2, 8
  N = n_lane * lanes
  g = torch.Generator().manual_seed(n_lane)
  z = (torch.randn(N, C, generator=g) + 1e2).float()
  if pivot_far:
    z[::n_lane] += 100.0
  z64 = z.double()
  parts = []
  for l in range(lanes):
    v = z[l * n_lane:(l + 1) * n_lane]
    p = v[0]
    s1 = torch.zeros(C, dtype=torch.float32); s2 = torch.zeros(C, dtype=torch.float32)
    for i in range(n_lane):
      d = v[i] - p
      s1 = s1 + d
      s2 = (d.double() * d.double() + s2.double()).float()           # fma
    nf = torch.tensor(float(n_lane), dtype=torch.float32)
    parts.append((nf, p + s1 / nf, torch.clamp(s2 - s1 * s1 / nf, min=0.0)))
  rn, rmean, rm2 = parts[0]
  for nf, mu, q in parts[1:]:                                          # stats_merge, fp32
    tot = rn + nf
    dl = mu - rmean
    rmean = rmean + dl * (nf / tot)
    rm2 = rm2 + q + dl * dl * (rn * nf / tot)
    rn = tot
  _, mu64, q64 = br.moments64(z64)
  s_mean, s_var = br.producer_scales(z64, n_lane, lanes, merges=8)
  e_mean = (rmean.double() - mu64).abs()
  e_var = (rm2.double() / N - q64 / N).abs()
  assert bool((e_mean <= 16 * br.U * s_mean).all()), (e_mean / (br.U * s_mean))
  assert bool((e_var <= 16 * br.U * s_var).all()), (e_var / (br.U * s_var))
  if n_lane == 16:
    sd = q64.div(N).sqrt()
    assert bool((1e4 * sd / N > 10 * 16 * br.U * s_mean).all())


def test_bwd_reference_branch_and_scales():
  """bn_bwd64's branch comes from the fp32 y; elements where an fma and two roundings disagree are flagged and priced; an
  fp32 evaluation of the backward stays within K = 16 of bwd_scales"""
  N, C = 4096, 3
  g = torch.Generator().manual_seed(11)
  z = (torch.randn(N, C, generator=g) * 3 + 100).float()
  g_a = (torch.randn(N, C, generator=g) + 50).float()
  mean = z.double().mean(0).float()
  invstd = (1.0 / torch.sqrt(z.double().var(0, unbiased=False) + br.EPS)).float()
  gamma = torch.tensor([1.0, 0.5, 2.0])
  scale, shift = invstd * gamma, -mean * invstd * gamma
  st = dict(mean=mean, invstd=invstd, scale=scale, shift=shift)
  ref = br.bn_bwd64(g_a, z, st, gamma)
  assert ref["amb"].dtype == torch.bool and ref["n_amb"] == int(ref["amb"].sum())
  # an fp32 backward with the fma branch
  pos = (z.double() * scale.double() + shift.double()).float() > 0
  g_y = torch.where(pos, g_a, g_a * br.SLOPE)
  xc = z - mean
  s_dy = g_y.double().sum(0).float(); s_dx = (g_y * xc).double().sum(0).float()
  g_z = gamma * invstd * (g_y - s_dy / N - xc * invstd * invstd * s_dx / N)
  sc = br.bwd_scales(g_a, z, st, gamma, ref, n_lane=64)
  for name, got in (("sum_dy", s_dy), ("sum_dx", s_dx), ("g_z", g_z)):
    err = (got.double() - ref[name]).abs()
    assert bool((err <= 16 * br.U * sc[name]).all()), name
  # a dropped element of the common-mode gradient moves sum_dy far beyond its bound
  assert bool((50.0 > 2 * 16 * br.U * sc["sum_dy"]).all())


def test_worst_ratio():
  assert br.worst_ratio(torch.tensor([1.0, 0.0]), torch.tensor([2.0, 0.0])) == 0.5
  assert br.worst_ratio(torch.tensor([1.0]), torch.tensor([0.0])) == float("inf")
