"""A plain float64 reference of train-mode BatchNorm (+ LeakyReLU) as the HIP kernels compute it, and the error models the GPU
tests (tests/test_gpu_batchnorm_fp64.py) bound the kernels with.  CPU only: nothing here imports the library.

Semantics are torch's: eps 1e-5, momentum 0.1, invstd from the biased variance, running_var from the unbiased one (the biased
one when the count is 1).  Tensors are channel-last: z is [..., C] (a PCL interior), partials are cnt [P], mean / m2 [P, C].

Every bound is  K * U * S:  U = 2^-24 (fp32 unit round-off), K a small fixed constant chosen by the test, S the scale of the
computation from the error model written next to the function that returns it (sums of absolute terms, never the result)."""
import math

import torch

U = 2.0 ** -24          # fp32 unit round-off
U64 = 2.0 ** -53        # fp64 unit round-off
EPS = 1e-5
MOMENTUM = 0.1
SLOPE = 0.2


def ulp32(x):
  """Spacing of fp32 numbers at |x| (float64 tensor): 2^(e - 23) for |x| in [2^e, 2^(e+1)), the denormal spacing near 0."""
  a = x.abs().double()
  e = torch.floor(torch.log2(a.clamp(min=2.0 ** -126)))
  return torch.pow(2.0, e - 23)


# ----------------------------------------------------------------------------- moments and merges
def moments64(z, groups=1):
  """(count, mean, M2) per channel of z [..., C] in float64; with groups > 1 the leading dimension is split into `groups`
  equal statistics groups (the trunk's left / right images) and every result gains a leading [groups] dimension."""
  C = z.shape[-1]
  if groups == 1:
    v = z.reshape(-1, C).double()
    mean = v.mean(0)
    return float(v.shape[0]), mean, ((v - mean) ** 2).sum(0)
  v = z.reshape(groups, -1, C).double()
  mean = v.mean(1)
  return torch.full((groups,), float(v.shape[1]), dtype=torch.float64), mean, ((v - mean[:, None]) ** 2).sum(1)


def chan_merge64(cnt, mean, m2):
  """The two-pass merge of partials cnt [P], mean / m2 [P, C]:  mean = sum n_i mean_i / N,  M2 = sum [M2_i + n_i (mean_i -
  mean)^2].  Empty partials (n_i = 0) contribute nothing, whatever their mean and M2 hold."""
  cnt, mean, m2 = cnt.double(), mean.double(), m2.double()
  live = cnt > 0
  cnt, mean, m2 = cnt[live], mean[live], m2[live]
  n = cnt.sum()
  mu = (cnt[:, None] * mean).sum(0) / n
  return float(n), mu, (m2 + cnt[:, None] * (mean - mu) ** 2).sum(0)


def bn_state64(count, mean, m2, gamma, beta, running_mean, running_var, eps=EPS, momentum=MOMENTUM):
  """torch's train-mode BatchNorm state from merged moments: mean, biased / unbiased variance, invstd, scale, shift and the
  updated running statistics, all float64."""
  gamma, beta = gamma.double(), beta.double()
  var_b = m2 / count
  var_u = m2 / (count - 1.0) if count > 1.0 else var_b
  invstd = 1.0 / torch.sqrt(var_b + eps)
  scale = gamma * invstd
  return dict(mean=mean, var=var_b, var_u=var_u, invstd=invstd, scale=scale, shift=beta - mean * scale,
              running_mean=momentum * mean + (1.0 - momentum) * running_mean.double(),
              running_var=momentum * var_u + (1.0 - momentum) * running_var.double())


def merge_bounds(cnt, mean, m2, gamma, state, c):
  """Absolute bounds of a merge that sums the partials in fp64 with a pivot K (the first non-empty partial's mean) and rounds
  its results once to fp32: 1 ulp of each fp32 result (2 where a result is formed from already rounded fp32 values), plus
  fp64 round-off  c * 2^-52 * S2/N  on the variance, where S2/N = var + (K - mean)^2 is what S2 - S1^2/S0 cancels from (c: the
  longest chain of additions), and c * 2^-52 * sum n_i |mean_i - K| / N on the mean."""
  cnt, mean, m2 = cnt.double(), mean.double(), m2.double()
  live = torch.nonzero(cnt > 0)[0, 0]
  K = mean[live]
  N = float(cnt.sum())
  e64 = c * 2.0 ** -52
  e_mean = e64 * ((cnt[:, None] * (mean - K).abs()).sum(0) / N + K.abs()) + ulp32(state["mean"])
  e_var = e64 * (state["var"] + (K - state["mean"]) ** 2)
  inv = state["invstd"]
  e_inv = 0.5 * inv ** 3 * e_var + ulp32(inv)
  g = gamma.double().abs()
  e_scale = g * e_inv + ulp32(state["scale"])
  e_shift = state["scale"].abs() * e_mean + state["mean"].abs() * e_scale + ulp32(state["mean"] * state["scale"]) + \
      ulp32(state["shift"])
  e_vu = e_var * (N / (N - 1.0) if N > 1.0 else 1.0) + ulp32(state["var_u"])
  return dict(mean=e_mean, invstd=e_inv, scale=e_scale, shift=e_shift, var_u=e_vu,
              running_mean=MOMENTUM * e_mean + ulp32(state["running_mean"]),
              running_var=MOMENTUM * e_vu + ulp32(state["running_var"]))


# ----------------------------------------------------------------------------- the producers' moments
def producer_scales(z, n_lane, lanes, merges):
  """Error scales (S_mean, S_var) [C] of fp32 moments of z [N, C] (float64 copy of the fp32 values the kernel stored) made
  the producers' way: every lane keeps shifted sums s1 = sum d, s2 = sum d^2 over at most `n_lane` elements (d = z - p, p the
  lane's first element) in fp32, mean_l = p + s1/n and M2_l = s2 - s1^2/n; a workgroup folds its lanes (or tiles) into one
  fp32 partial with `merges` pairwise Chan merges; the partials are merged in fp64.

  Recursive fp32 summation of n terms errs by at most n u sum|d|, so the lane sums err by n_l u sum|d| and n_l u sum d^2
  (s1^2/n adds at most that much again: (sum|d|)^2/n <= sum d^2).  With |d| <= |z - m| + |p - m|, and the pivots being at most
  `lanes` distinct elements of the channel, the sum over lanes is bounded without knowing which lane held which element:
      sum_l n_l sum_{i in l} |d_i|  <=  n_l sum|z - m| + n_l^2 top_lanes(|z - m|)      (top_P: sum of the P largest)
  and with d^2 <= 2 (z - m)^2 + 2 (p - m)^2 the same for d^2.  The fp32 fold adds `merges` roundings of |mean_l| and of M2;
  an error e_l in mean_l moves the merge's n_l (mean_l - m)^2 by 2 n_l |mean_l - m| e_l <= 2 n_l R e_l (R = max |z - m|).
      S_mean = [n_l sum|z-m| + n_l^2 top(|z-m|)] / N + merges mean|z|
      S_var  = [n_l (2 sum(z-m)^2 + 2 n_l top((z-m)^2)) + merges sum (z-m)^2] / N + 2 R S_mean"""
  z = z.reshape(-1, z.shape[-1]).double()
  N = z.shape[0]
  m = z.mean(0)
  d = z - m
  ad, d2 = d.abs(), d * d
  P = min(int(lanes), N)
  top1 = ad.topk(P, dim=0).values.sum(0)
  top2 = d2.topk(P, dim=0).values.sum(0)
  s_mean = (n_lane * ad.sum(0) + n_lane * n_lane * top1) / N + merges * z.abs().mean(0)
  s_var = (n_lane * (2.0 * d2.sum(0) + 2.0 * n_lane * top2) + merges * d2.sum(0)) / N + 2.0 * ad.max(0).values * s_mean
  return s_mean, s_var


# ----------------------------------------------------------------------------- backward
def lrelu_branch(z, scale, shift):
  """(positive, ambiguous): the LeakyReLU branch y = z*scale + shift > 0 the kernels take, from the fp32 y formed with one
  rounding (an fma), and the elements whose sign differs when y is formed as fp32(fp32(z*scale) + shift) instead."""
  z32, sc, sh = z.float(), scale.float(), shift.float()
  y_fma = (z32.double() * sc.double() + sh.double()).float()       # the product is exact in fp64: one rounding, as an fma
  y_two = z32 * sc + sh                                            # two roundings
  pos = y_fma > 0
  return pos, pos != (y_two > 0)


def bn_bwd64(g_a, z, state, gamma, slope=SLOPE):
  """The train-mode BatchNorm + LeakyReLU backward in float64 with the state the kernel used (fp32 mean / invstd / scale /
  shift).  g_a, z: [N, C].  Returns g_y = g_a lrelu'(y), sum g_y, sum g_y (z - mean), g_gamma, g_beta, g_z, and `amb`: the
  elements whose branch depends on whether y was formed with an fma (either branch is allowed there; see lrelu_branch)
  with `amb_ga` = sum over them of |g_a| (1 - slope) per channel, by how much a sum can move."""
  g_a, z = g_a.reshape(-1, g_a.shape[-1]).double(), z.reshape(-1, z.shape[-1]).double()
  N = z.shape[0]
  mean, invstd = state["mean"].double(), state["invstd"].double()
  pos, amb = lrelu_branch(z, state["scale"], state["shift"])
  g_y = torch.where(pos, g_a, g_a * slope)
  xc = z - mean
  s_dy, s_dx = g_y.sum(0), (g_y * xc).sum(0)
  g_gamma, g_beta = s_dx * invstd, s_dy
  g_z = gamma.double() * invstd * (g_y - s_dy / N - xc * invstd * invstd * s_dx / N)
  amb_ga = torch.where(amb, g_a.abs() * (1.0 - slope), torch.zeros_like(g_a)).sum(0)
  return dict(g_y=g_y, sum_dy=s_dy, sum_dx=s_dx, g_gamma=g_gamma, g_beta=g_beta, g_z=g_z, amb=amb, amb_ga=amb_ga,
              n_amb=int(amb.sum()))


def bwd_scales(g_a, z, state, gamma, ref, n_lane, slope=SLOPE):
  """Error scales of the backward's fp32 computation.  Stage 1 sums g_y and g_y (z - mean) per lane over at most n_lane
  elements in fp32 ((z - mean) itself rounded: u |z - mean|), then in fp64:
      S_dy = n_l sum|g_y|,   S_dx = n_l sum|g_y| (|z - mean| + |z| + |mean|)          (+ the ambiguous branches: amb_ga)
  Stage 3, g_z = gamma invstd (g_y - c1 - (z - mean) invstd^2 c2), c1 = sum g_y / N, c2 = sum g_y (z - mean) / N, in fp32: a
  few roundings of every term, the fp32 (z - mean) term (|z| + |mean|) invstd and the errors of c1, c2:
      S_gz = |gamma| invstd (|g_y| + |c1| + S_dy/N + (|z - m| + |z| + |m|) invstd^2 (|c2| + S_dx/N))"""
  g_a, z = g_a.reshape(-1, g_a.shape[-1]).double(), z.reshape(-1, z.shape[-1]).double()
  N = z.shape[0]
  mean, invstd = state["mean"].double(), state["invstd"].double()
  ag = ref["g_y"].abs()
  spread = (z - mean).abs() + z.abs() + mean.abs()
  s_dy = n_lane * ag.sum(0) + ref["amb_ga"] / U
  s_dx = n_lane * (ag * spread).sum(0) + ref["amb_ga"] * spread.max(0).values / U
  c1, c2 = ref["sum_dy"].abs() / N, ref["sum_dx"].abs() / N
  s_gz = gamma.double().abs() * invstd * (ag + c1 + s_dy / N + spread * invstd * invstd * (c2 + s_dx / N))
  return dict(sum_dy=s_dy, sum_dx=s_dx, g_gamma=s_dx * invstd + ref["sum_dx"].abs() * invstd, g_beta=s_dy, g_z=s_gz)


def worst_ratio(err, bound):
  """max err / bound over finite entries (0 where both are 0)."""
  err, bound = err.double(), bound.double()
  r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, math.inf), err))
  return float(r.max()) if r.numel() else 0.0
