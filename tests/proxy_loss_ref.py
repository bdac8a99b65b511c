"""numpy float32 restatement of csrc/proxy_loss.hip (as_proxy_term_fwd / as_proxy_term_bwd), the contract of
include/adaptive_stereo_hip.h op by op: the same chain per pixel in float32, math.fsum for the sums.

  labelled   code == 0 and disp > 0            (NaN, -0.0, 0.0, negatives and every non-zero code: no label)
  d = disp - pred,  v = sqrt(d * d + 4) / 2 - 1 (every operation rounded to float32),  e = |d|
  S = sum v, C = count, E = sum e, B = count(e > bad_px) over the labelled pixels
  out6 = [f32(S) / f32(max(C, 1)), max(C, 1), f32(S), f32(E / max(C, 1)), f32(B / max(C, 1)), C]
  g_pred = (g_loss / out6[1]) * -d / (2 sqrt(d * d + 4)) on the labelled pixels, 0 elsewhere

What the device runs for v (csrc/khamis.h, the chain of khamis_fwd_kernel, read from the compiled code) is fma(d, d, 4), the
hardware's square root (within an ulp of the root, where numpy's is correctly rounded) and fma(s, 0.5, -1): three roundings
against the five here.  Per pixel the two chains were seen two ulps of v apart at d = 2.9999998; by their roundings they can
differ by up to 3.25 ulps of v + 1.  Counts, e and everything formed from them are exact arithmetic and agree to the last bit.
The backward is different: as_khamis_bwd and as_proxy_term_bwd compile without contraction and with IEEE division and square
root, which is exactly ``backward`` below, bit for bit.

``wrong`` names a plausible mistake (WRONG); tests/test_proxy_loss_ref_cpu.py tells each from the contract by a named case.
"""
import math

import numpy as np

F = np.float32
WRONG = ("bad_ge", "disp_ge_zero", "ignore_code", "raw_count_denominator")


def labelled(disp, code, wrong=None):
  disp, code = np.asarray(disp, dtype=F).reshape(-1), np.asarray(code, dtype=np.uint8).reshape(-1)
  with np.errstate(invalid="ignore"):
    positive = disp >= 0 if wrong == "disp_ge_zero" else disp > 0
  return positive if wrong == "ignore_code" else positive & (code == 0)


def materialised_labels(disp, code):
  """where(code == 0, disp, 0): what sgm.ProxyLabeler writes and the supervised path reads with gt > 0"""
  disp = np.asarray(disp, dtype=F)
  return np.where(np.asarray(code, dtype=np.uint8).reshape(disp.shape) == 0, disp, F(0)).astype(F)


def pixel_terms(pred, disp, code, wrong=None):
  """(mask, v float32, e float32) over the flattened maps; v and e are 0 off the label set"""
  pred, disp = np.asarray(pred, dtype=F).reshape(-1), np.asarray(disp, dtype=F).reshape(-1)
  m = labelled(disp, code, wrong)
  with np.errstate(invalid="ignore", over="ignore"):
    d = (np.where(m, disp, F(0)) - np.where(m, pred, F(0))).astype(F)
    v = ((np.sqrt(((d * d).astype(F) + F(4)).astype(F)).astype(F) / F(2)).astype(F) - F(1)).astype(F)
    e = np.abs(d).astype(F)
  return m, np.where(m, v, F(0)).astype(F), np.where(m, e, F(0)).astype(F)


def forward(pred, disp, code, bad_px, wrong=None):
  """out6 as float32 [6]"""
  m, v, e = pixel_terms(pred, disp, code, wrong)
  count = int(m.sum())
  nv = count if wrong == "raw_count_denominator" else max(count, 1)
  S = math.fsum(v[m].astype(np.float64).tolist())
  E = math.fsum(e[m].astype(np.float64).tolist())
  with np.errstate(invalid="ignore"):
    B = int(((e >= F(bad_px)) if wrong == "bad_ge" else (e > F(bad_px)))[m].sum())
  with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
    loss = F(S) / F(nv)
    return np.array([loss, F(max(count, 1)), F(S), F(np.float64(E) / nv), F(np.float64(B) / nv), F(count)], dtype=F)


def backward64(pred, disp, code, g_loss, wrong=None):
  """float64 [n]: g_loss / max(C, 1) * -d / (2 sqrt(d^2 + 4)) from the float32 inputs, 0 off the label set"""
  pred, disp = np.asarray(pred, dtype=F).reshape(-1), np.asarray(disp, dtype=F).reshape(-1)
  m = labelled(disp, code, wrong)
  d = np.where(m, disp.astype(np.float64), 0.0) - np.where(m, pred.astype(np.float64), 0.0)
  return np.where(m, float(g_loss) / max(int(m.sum()), 1) * -d / (2.0 * np.sqrt(d * d + 4.0)), 0.0)


def backward(pred, disp, code, g_loss, out6):
  """float32 [n], the kernel's operation order, each operation rounded: scale = g_loss / out6[1];
  g = -scale * d / (2 * sqrt(d * d + 4)).  as_khamis_bwd and as_proxy_term_bwd are compiled under `fp contract(off)` with
  correctly rounded division and square root: their results are these bits (tests/test_gpu_proxy_loss.py pins both).
  as_khamis2_bwd is not: supervised.hip contracts d * d + 4, as it always did."""
  pred, disp = np.asarray(pred, dtype=F).reshape(-1), np.asarray(disp, dtype=F).reshape(-1)
  m = labelled(disp, code)
  scale = F(g_loss) / F(out6[1])
  with np.errstate(invalid="ignore", over="ignore"):
    d = (np.where(m, disp, F(0)) - np.where(m, pred, F(0))).astype(F)
    inner = ((d * d).astype(F) + F(4)).astype(F)
    g = ((-scale * d).astype(F) / (F(2) * np.sqrt(inner).astype(F)).astype(F)).astype(F)
  return np.where(m, g, F(0)).astype(F)


def planted_case(n, seed, density=0.6):
  """pred, disp, code of n pixels with every kind of not-a-label mixed in: codes 1..7 over positive disparities, and under code
  0 NaN, -0.0, 0.0 and negatives"""
  rng = np.random.default_rng(seed)
  pred = (rng.random(n) * 60.0).astype(F)
  disp = (pred + rng.normal(0.0, 2.5, n)).astype(F)
  disp = np.where(disp <= 0, F(0.25), disp).astype(F)
  code = np.where(rng.random(n) < density, 0, rng.integers(1, 8, n)).astype(np.uint8)
  odd = rng.random(n) < 0.08
  kinds = rng.integers(0, 4, n)
  disp = np.where(odd & (kinds == 0), F(np.nan), disp)
  disp = np.where(odd & (kinds == 1), F(-0.0), disp)
  disp = np.where(odd & (kinds == 2), F(0.0), disp)
  disp = np.where(odd & (kinds == 3), -disp, disp).astype(F)
  return pred, disp, code
