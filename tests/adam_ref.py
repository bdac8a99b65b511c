"""fp64 reference of one step of global-norm clip + Adam (csrc/optim.hip: as_sumsq_clip, as_adam_step), from a given state.

    coef   = min(max_norm / (sqrt(sum g^2) + 1e-6), 1)                      torch.nn.utils.clip_grad_norm_
    g      = g * coef                                                        (stored in the gradient's own dtype, as torch does)
    m'     = m + (1 - b1) (g - m)                                            torch.optim.Adam, single-tensor path
    v'     = b2 v + (1 - b2) g g
    update = -(lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)

Two sets of hyper-parameters.  ``hyper(..., f32=False)`` keeps the Python doubles: that is torch.optim.Adam, and the CPU test
pins it to the real optimizer in float64.  ``hyper(..., f32=True)`` rounds each of lr, b1, b2, eps to float32 first, because that
is what the library's C ABI receives: the kernel forms ``1.f - b2`` from ``0.999f`` (exact in float32 for any b in [0.5, 1]) and
its bias corrections from ``pow((double)b, step)``.  The two differ, and the difference is the library's documented deviation
from torch: the weight of ``g g`` by ``rel_1m(b2) = |(1 - b2_f32) - (1 - b2)| / (1 - b2)`` (1.29e-5 for 0.999), the update by at
most half of that once the bias correction is built from the same rounded b2.  The GPU test compares the kernel with the
float32-hyper-parameter form, the CPU test pins the distance between the two.

Bounds for a float32 evaluation of one step, ``U = 2^-24``, each rounding counted from adam_kernel's expressions:

* ``m'``: subtract, multiply, add -> ``3 U (|m| + (1 - b1) |g - m|)``;
* ``v'``: ``((1 - b2) g) g`` two roundings and the add, ``b2 v`` one and the add -> ``3 U (b2 |v| + (1 - b2) g g)``;
* update, from the *stored* float32 m' and v' (their own error is judged above, so each bound is a one-step bound):
  ``K_UPDATE U |update| + ulp32(p_after) / 2`` with K_UPDATE = 8: bc1 to float, lr / bc1, sqrt, bc2_sqrt to float,
  the division by it, the addition of eps, m' / denom, the product with the step size; the half ulp is the final subtraction
  from p.
"""
import math

import torch

U = 2.0 ** -24
K_STATE = 3
K_UPDATE = 8
F32, F64 = torch.float32, torch.float64


def f32(x):
  return float(torch.tensor(float(x), dtype=F32))


def hyper(lr, b1, b2, eps, as_f32):
  """(lr, b1, b2, eps) as Python floats: as given, or each rounded to float32 (what the C ABI receives)"""
  return tuple(f32(x) for x in (lr, b1, b2, eps)) if as_f32 else (float(lr), float(b1), float(b2), float(eps))


def rel_1m(b):
  """relative difference of (1 - float32(b)) from (1 - b): how far the weight of the new term moves when b arrives as float32"""
  return abs((1.0 - f32(b)) - (1.0 - b)) / (1.0 - b)


def clip_coef(sumsq, max_norm):
  """clip_grad_norm_'s coefficient in float64"""
  return min(max_norm / (math.sqrt(sumsq) + 1e-6), 1.0)


def clip_coef32(sumsq32, max_norm):
  """the same expression in float32 on the CPU, from a float32 sum of squares (0-dim tensor) -> 0-dim float32 tensor; sqrt and
  divide are correctly rounded, so a device that rounds them correctly too gives the same bits"""
  s = sumsq32.detach().cpu().to(F32).reshape(())
  c = torch.tensor(float(max_norm), dtype=F32) / (torch.sqrt(s) + torch.tensor(1e-6, dtype=F32))
  return torch.minimum(c, torch.tensor(1.0, dtype=F32))


def bias_corrections(b1, b2, t):
  return 1.0 - math.pow(b1, t), 1.0 - math.pow(b2, t)


def moments(g, m, v, hp):
  """-> (m', v', terms of m', terms of v') in float64; g is the gradient Adam sees (already clipped)"""
  _, b1, b2, _ = hp
  g, m, v = g.double(), m.double(), v.double()
  m1 = m + (1.0 - b1) * (g - m)
  v1 = b2 * v + (1.0 - b2) * g * g
  return m1, v1, m.abs() + (1.0 - b1) * (g - m).abs(), b2 * v.abs() + (1.0 - b2) * g * g


def update(m1, v1, t, hp):
  """p_after - p_before in float64 from the new moments"""
  lr, b1, b2, eps = hp
  bc1, bc2 = bias_corrections(b1, b2, t)
  return -(lr / bc1) * (m1.double() / (torch.sqrt(v1.double()) / math.sqrt(bc2) + eps))


def step(p, g, m, v, t, hp):
  """one Adam step in float64 -> dict(p, m, v, update)"""
  m1, v1, _, _ = moments(g, m, v, hp)
  upd = update(m1, v1, t, hp)
  return dict(p=p.double() + upd, m=m1, v=v1, update=upd)


def ulp32(x):
  """spacing of binary32 at |x| -> float64 (the smallest normal's spacing below it)"""
  e = torch.frexp(x.float().abs().clamp_min(2.0 ** -126)).exponent.double()
  return torch.pow(2.0, e - 24.0)
