"""A plain float64 restatement (numpy) of what csrc/confidence.hip and the confidence gate of csrc/pointcloud.hip compute, written
from the contract in include/adaptive_stereo_hip.h: the three confidence maps of a logits volume, the gate on the point cloud,
the binned error statistics; the bound of every output; and the cases the GPU file (tests/test_gpu_confidence.py) runs.  CPU
only: nothing here imports the library.  tests/test_confidence_ref_cpu.py holds the restatements to torch's float64 soft-max,
brackets a float32 emulation of the written op order with the bounds and shows that the cases tell deliberately wrong
restatements (MUTANTS) from the right one.  The reference project has no counterpart, so there is no fixture: the oracle is fp64
arithmetic from the definitions.

Bounds follow tail_ref's rule, derived and never tuned (U = 2^-24, gamma(n) for a sum of n terms in any order, K_EXP ulps for the
device's expf, TINY the smallest normal number).  With p the fp64 soft-max of the kernel's OWN fp32 inputs, x_d = l_d - m1 (exact
in fp64; the fp32 subtraction rounds once), se = sum_d exp(x_d), H = ln se - sum_d p_d x_d the entropy:
  eps_d   = (|x_d| + 2 K_EXP) U              the rounded subtraction, magnified by exp, and expf itself
  eps_se  = sum_d p_d eps_d + gamma(D)       the sum of the exponentials
  pmax    = 1 / se:                           e = pmax (eps_se + U)                                  (the quotient: U)
  mass    = near / se:                        e = sum_near p_d eps_d + mass (gamma(3) + eps_se + U)
  T / se  = sum_d p_d x_d:                    each product e_d t_d errs by eps_d (e_d), U (t_d, the rounded subtraction) and U (the
                                              product); the sum by gamma(D); the quotient by eps_se + U
  ln se:                                      eps_se through the argument, K_LOG ulps of logf
  e_H     = sum_d p_d |x_d| (eps_d + 2 U) + (gamma(D) + eps_se + U) sum_d p_d |x_d| + eps_se + K_LOG U |ln se| + U |H|
  cent    = 1 - H / ln D:                     e = e_H / ln D + (H / ln D) (K_LOG + 1) U + U |cent|   (logf(D), the quotient, the
                                              subtraction; the clamp to [0, 1] moves a value towards the reference, which lies there)
K_LOG = 2 is the one new number: 1 ulp for a library logf and the same again as margin, the rule K_EXP follows.  Not fitted.

Underflow (tail_ref's term).  An exponential below TINY comes out denormal or zero, wrong by at most TINY in absolute terms: se
(>= 1) and the window sum gain D TINY and 3 TINY, so pmax and mass gain (D + 3) TINY.  In T the product of such an e_d with t_d
errs by at most TINY |t_d| + TINY while expf(t_d) is not zero (|t_d| < 104), and where it is zero the contract drops a term whose
true size e^-|x| |x| is below 104 TINY: e_H gains 106 D TINY.  (1e-36: it matters only where the bound itself would be 0.)

D == 1: the three maps are exactly 1 (bound 0).  A bad column (a NaN, a +inf, or nothing but -inf) is the quiet NaN in every map.
abs_err[k] of the histogram is an fp64 sum of at most n non-negative fp32 terms in any order: n 2^-53 times the bin's own sum."""
import math

import numpy as np

import ood_ref
import pointcloud_ref as pr
from tail_ref import U, gamma_n, K_EXP, TINY

K_LOG = 2                 # ulps of the device's logf: 1 for a library logf + 1 of margin (not fitted)
F = np.float32
QNAN_BITS = 0x7FC00000
SHAPES, GAINS = ood_ref.SHAPES, ood_ref.GAINS
MAP_NAMES = ("pmax", "cent", "mass")

# planted columns: all in image 0, on its LAST pixels (ood_ref.make_volume plants its own on the first six)
PLANT_KINDS = ("all_equal", "max_both_ends", "mode_last", "two_peaks", "one_hot_200", "minus_inf", "all_minus_inf", "plus_inf",
               "nan")
BAD_KINDS = ("all_minus_inf", "plus_inf", "nan")


def case_name(shape, gain):
  return ood_ref.case_name(shape, gain)


def planted(shape):
  """{kind: (b, pixel)} of the columns make_volume adds to ood_ref's own (those need H * W >= 15 to stay clear of them)."""
  B, D, H, W = shape
  out = {}
  if H * W < 6 + len(PLANT_KINDS):
    return out
  for i, kind in enumerate(PLANT_KINDS):
    if kind == "two_peaks" and D < 4:
      continue
    if kind in ("max_both_ends", "mode_last", "minus_inf") and D < 2:
      continue
    out[kind] = (0, H * W - 1 - i)
  return out


def make_volume(shape, gain):
  """ood_ref.make_volume (its planted ties and its NaN included) + the planted columns of this file."""
  B, D, H, W = shape
  g = F(gain)
  vol = ood_ref.make_volume(shape, gain)
  flat = vol.reshape(B, D, H * W)
  for kind, (b, p) in planted(shape).items():
    top = np.abs(flat[b, :, p]).max()
    if kind == "all_equal":
      flat[b, :, p] = F(0.75) * g
    elif kind == "max_both_ends":                     # the first index wins; the window is clipped at d = 0
      flat[b, 0, p] = flat[b, D - 1, p] = top + g
    elif kind == "mode_last":                         # the window is clipped at d = D - 1
      flat[b, D - 1, p] = top + F(2) * g
    elif kind == "two_peaks":                         # two equal peaks D/2 apart: the soft-argmax lies between them
      flat[b, 1, p] = flat[b, 1 + D // 2, p] = top + g
    elif kind == "one_hot_200":
      flat[b, :, p] = F(0)
      flat[b, D // 3, p] = F(200)
    elif kind == "minus_inf":                         # legal: probability 0
      flat[b, D // 2, p] = -np.inf
    elif kind == "all_minus_inf":
      flat[b, :, p] = -np.inf
    elif kind == "plus_inf":
      flat[b, D // 2, p] = np.inf
    elif kind == "nan":
      flat[b, D - 1, p] = np.nan
  return vol


def bad_columns(vol):
  """[B,H,W] bool: a NaN, a +inf, or nothing but -inf"""
  return np.isnan(vol).any(axis=1) | (vol == np.inf).any(axis=1) | (vol == -np.inf).all(axis=1)


# ---- the three maps -----------------------------------------------------------------------------------------------------------
def maps(vol, dtype=np.float64, mut=None, exp=np.exp, log=np.log):
  """pmax, cent, mass [B,H,W] of fp32 logits [B,D,H,W] in the written op order, every operation in `dtype` (float64: the
  reference; float32: an emulation of the kernel, one rounding per operation), NaN at bad columns; also a (the first index of the
  maximum) and, in float64, the pieces the bounds need.
  mut:  "last_max"      the LAST maximum wins a tie
        "window_2"      the window of mass is +-2
        "entropy_raw"   the entropy is not divided by ln D
        "no_max"        the exponentials are taken without subtracting the maximum
        "zero_times_t"  e * t is taken where e == 0"""
  vol = np.asarray(vol)
  assert vol.dtype == np.float32 and vol.ndim == 4
  B, D, H, W = vol.shape
  x = vol.astype(dtype)
  bad = bad_columns(vol)
  with np.errstate(all="ignore"):
    m1 = np.full((B, H, W), -np.inf, dtype)
    a = np.zeros((B, H, W), np.int64)
    for d in range(D):
      gt = (x[:, d] >= m1) if mut == "last_max" else (x[:, d] > m1)
      m1 = np.where(gt, x[:, d], m1)
      a = np.where(gt, d, a)
    shift = np.zeros_like(m1) if mut == "no_max" else m1
    t = (x - shift[:, None]).astype(dtype)
    e = exp(t).astype(dtype)
    se, T = np.zeros((B, H, W), dtype), np.zeros((B, H, W), dtype)
    for d in range(D):
      se = (se + e[:, d]).astype(dtype)
      prod = (e[:, d] * t[:, d]).astype(dtype)
      T = (T + (prod if mut == "zero_times_t" else np.where(e[:, d] == 0, dtype(0), prod))).astype(dtype)

    def take(k):
      i = a + k
      v = np.take_along_axis(e, np.clip(i, 0, D - 1)[:, None], axis=1)[:, 0]
      return np.where((i >= 0) & (i < D), v, dtype(0))
    near = ((take(-1) + take(0)).astype(dtype) + take(1)).astype(dtype)
    if mut == "window_2":
      near = ((near + take(-2)).astype(dtype) + take(2)).astype(dtype)
    pmax = (dtype(1) / se).astype(dtype)
    mass = (near / se).astype(dtype)
    Hn = (log(se).astype(dtype) - (T / se).astype(dtype)).astype(dtype)
    if D == 1:
      pmax, mass, cent = (np.ones((B, H, W), dtype) for _ in range(3))
    else:
      q = Hn if mut == "entropy_raw" else (Hn / log(dtype(D)).astype(dtype)).astype(dtype)
      cent = np.minimum(np.maximum((dtype(1) - q).astype(dtype), dtype(0)), dtype(1))
  nan = np.array([QNAN_BITS], np.uint32).view(F)[0].astype(dtype)
  out = dict(pmax=np.where(bad, nan, pmax), cent=np.where(bad, nan, cent), mass=np.where(bad, nan, mass), a=a, bad=bad)
  if dtype == np.float64 and mut is None:
    out.update(x=t, p=e / se[:, None], se=se, H=Hn)
  return out


def stage(vol):
  """maps(vol) in float64 and the bound of each map (see the module docstring): e_pmax, e_cent, e_mass, 0 for D == 1 and NaN at
  bad columns (they are compared by their bits)."""
  r = maps(vol)
  B, D, H, W = vol.shape
  if D == 1:
    for k in MAP_NAMES:
      r["e_" + k] = np.where(r["bad"], np.nan, 0.0)
    return r
  with np.errstate(all="ignore"):
    p, x = r["p"], r["x"]
    live = p > 0                                                  # a -inf (or an exponential that is 0 in fp64) has no share
    ax = np.where(live, np.abs(x), 0.0)
    eps_d = (ax + 2.0 * K_EXP) * U
    eps_se = (p * eps_d).sum(1) + gamma_n(D)
    dd = np.arange(D).reshape(1, D, 1, 1)
    near = np.abs(dd - r["a"][:, None]) <= 1
    r["e_pmax"] = r["pmax"] * (eps_se + U) + (D + 3) * TINY
    r["e_mass"] = (np.where(near, p * eps_d, 0.0)).sum(1) + r["mass"] * (gamma_n(3) + eps_se + U) + (D + 3) * TINY
    spx = (p * ax).sum(1)
    e_H = (p * ax * (eps_d + 2.0 * U)).sum(1) + (gamma_n(D) + eps_se + U) * spx + eps_se + K_LOG * U * np.abs(np.log(r["se"])) + \
        U * np.abs(r["H"]) + 106.0 * D * TINY
    lnD = math.log(D)
    r["e_H"] = e_H
    r["e_cent"] = e_H / lnD + (r["H"] / lnD) * (K_LOG + 1) * U + U * np.abs(r["cent"])
  for k in MAP_NAMES:
    r["e_" + k] = np.where(r["bad"], np.nan, r["e_" + k])
  return r


def worst_ratio(got, ref, bound, bad):
  """worst |got - ref| / bound over the good columns (0 / 0 counts as 0, anything / 0 as infinite); infinite when a good column
  holds a NaN or a bad one anything but the quiet NaN 0x7FC00000 (float32 input; a NaN of any kind otherwise)"""
  got = np.ascontiguousarray(got).reshape(ref.shape)
  wrong_nan = (got.view(np.uint32)[bad] != QNAN_BITS).any() if got.dtype == np.float32 else not np.isnan(got[bad]).all()
  if wrong_nan or np.isnan(got[~bad]).any():
    return float("inf")
  err = np.abs(got.astype(np.float64) - ref)[~bad]
  b = bound[~bad]
  with np.errstate(all="ignore"):
    r = np.where(err == 0, 0.0, np.where(b > 0, err / b, np.inf))
  return float(r.max()) if r.size else 0.0


MUTANTS = {
  "the last maximum wins a tie": "last_max",
  "a window of +-2": "window_2",
  "entropy not normalised": "entropy_raw",
  "no maximum subtracted": "no_max",
  "e * t taken at e == 0": "zero_times_t",
}


# ---- the gate -----------------------------------------------------------------------------------------------------------------
def gate(p, conf, conf_min):
  """pointcloud_ref.points() with `valid &= conf >= conf_min` (one fp32 compare: a NaN confidence fails, +inf passes): a new
  dict for pointcloud_ref.organized() / voxel_cloud(), and rejected [B], the pixels valid by depth that failed the gate."""
  conf = np.asarray(conf)
  assert conf.dtype == np.float32 and conf.shape == p["valid"].shape
  with np.errstate(invalid="ignore"):
    keep = conf >= F(conf_min)
  q = dict(p)
  q["valid"] = p["valid"] & keep
  return q, (p["valid"] & ~keep).reshape(keep.shape[0], -1).sum(axis=1)


# ---- the histogram ------------------------------------------------------------------------------------------------------------
def bin_scale(K, lo, hi):
  return F(float(K) / (float(hi) - float(lo)))


def sparsify_loop(key, pred, gt, lo, scale, K, tau):
  """A plain loop over the elements, every operation in fp32 as written; abs_err per bin by math.fsum (exact, rounded once).
  Returns dict(count [K], bad [K] int64, abs_err [K] float64, skipped)."""
  lo, scale, tau = F(lo), F(scale), F(tau)
  count, bad, terms, skipped = [0] * K, [0] * K, [[] for _ in range(K)], 0
  with np.errstate(all="ignore"):
    for kv, pv, gv in zip(np.asarray(key, F).ravel(), np.asarray(pred, F).ravel(), np.asarray(gt, F).ravel()):
      if not (gv > 0):
        continue
      err = np.abs(F(pv - gv))
      if np.isnan(kv) or np.isnan(err):
        skipped += 1
        continue
      t = F(F(kv - lo) * scale)
      k = 0 if t < 0 else (K - 1 if t >= F(K) else int(t))
      count[k] += 1
      bad[k] += int(err > tau)
      terms[k].append(float(err))
  return dict(count=np.array(count, np.int64), bad=np.array(bad, np.int64),
              abs_err=np.array([math.fsum(v) for v in terms], np.float64), skipped=skipped)


def abs_err_bound(n, abs_err):
  return float(n) * 2.0 ** -53 * np.asarray(abs_err, np.float64)


SPARSE_N = [1, 63, 64, 65, 4099]
SPARSE_K = [1, 2, 256, 1024]


def _below(x):
  return np.nextafter(F(x), F(-np.inf), dtype=F)


def sparsify_case(n, K, seed=0):
  """key, pred, gt [n] fp32 for lo = 0, scale = K: keys exactly k / K and their fp32 neighbours below (bin k and bin k - 1), keys
  below lo and above hi (the end bins), NaN keys, NaN predictions and elements without ground truth (0, negative, NaN), and
  errors on either side of tau = 3; element 0 is always an ordinary one."""
  rs = np.random.RandomState(7919 * n + K + seed)
  ks = rs.randint(0, K + 1, n)
  edge = (ks.astype(np.float64) / K).astype(F)                 # k / K rounded to fp32 once
  key = np.where(rs.rand(n) < 0.5, edge, _below(edge)).astype(F)
  gt = (1.0 + 60.0 * rs.rand(n)).astype(F)
  err = np.where(rs.rand(n) < 0.5, 3.0 * rs.rand(n), 3.0 + 20.0 * rs.rand(n)).astype(F)
  err[rs.rand(n) < 0.1] = F(3.0)                                # exactly tau is not bad (when the subtraction is exact)
  pred = (gt + err * np.where(rs.rand(n) < 0.5, 1, -1).astype(F)).astype(F)
  kind = rs.randint(0, 16, n)
  kind[0] = 15
  key[kind == 0] = F(-0.25)
  key[kind == 1] = F(1.5)
  key[kind == 2] = F(np.inf)
  key[kind == 3] = F(-np.inf)
  key[kind == 4] = F(np.nan)
  pred[kind == 5] = F(np.nan)
  gt[kind == 6] = F(0)
  gt[kind == 7] = F(-2)
  gt[kind == 8] = F(np.nan)
  return key, pred, gt


# ---- curves (what adaptive_stereo.confidence computes on the host, as a plain loop) -------------------------------------------
def curve_loop(count, bad, abs_err, remove="low"):
  K = len(count)
  order = list(range(K)) if remove == "low" else list(range(K - 1, -1, -1))
  total = float(sum(int(c) for c in count))
  frac, epe, d1 = [], [], []
  for j in range(K + 1):
    rest = order[j:]
    n = float(sum(int(count[k]) for k in rest))
    frac.append((total - n) / total if total > 0 else 0.0)
    epe.append(math.fsum(float(abs_err[k]) for k in rest) / n if n > 0 else 0.0)
    d1.append(float(sum(int(bad[k]) for k in rest)) / n if n > 0 else 0.0)
  return np.array(frac), np.array(epe), np.array(d1)
