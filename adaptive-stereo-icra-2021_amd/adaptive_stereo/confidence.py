"""Per-pixel confidence of the coarse disparity, and the sparsification statistics that calibrate a gate on it
(csrc/confidence.hip).

The network's post-aggregation matching distribution says where it does not know; the library computes it on every forward pass
and otherwise uses only its image mean (the OOD gate).  Here it reaches the pixel:

  conf = disparity_confidence(outputs["cost_volume_l/4"])         # {"pmax", "entropy", "mass"}: [B,Hc,Wc], one launch
  cloud = proj.voxel_cloud(outputs["pred_disp_l/0"], left, confidence=conf["mass"], conf_min=0.8)   # pointcloud.DepthProjector

and a threshold is chosen from a validation split with ground truth, as ood.py chooses --ood_threshold:

  by_conf, by_err = SparsificationCollector(), SparsificationCollector(hi=192.0)
  full = upsample_confidence(conf["mass"], H, W)
  by_conf.add(full, pred, gt)                                      # enqueues only: graph-capturable
  by_err.add((pred - gt).abs(), pred, gt)                          # the oracle: the error itself as the key
  area = ause(by_conf.curve("low"), by_err.curve("high"))

The arithmetic of the maps and of the bins is fixed op by op in include/adaptive_stereo_hip.h; the host halves (curve, ause) are
plain numpy in fp64.  The reference has no counterpart.
"""
import numpy as np
import torch

from . import _native as nat
from .collect import check_f32, gpu_device

KINDS = ("pmax", "entropy", "mass", "fcs")
MAX_BINS = 1024


def _check_volume(cost_volume):
  check_f32("adaptive_stereo.confidence", "cost_volume", cost_volume, ((4,), "[B,D,H,W]"))
  return cost_volume.detach()


def disparity_confidence(cost_volume, kinds=("pmax", "entropy", "mass")):
  """{kind: [B,Hc,Wc]} of a logits volume [B,D,Hc,Wc] (the ``cost_volume_{side}/{scale}`` output as it is).  Never synchronises.
    "pmax"     the soft-max probability of the mode
    "entropy"  one minus the normalised entropy of the soft-max, in [0, 1]
    "mass"     the probability within one coarse disparity of the mode
    "fcs"      the max-minus-mean feature-contrast map in its raw units (as_fcs_scores' mean map), not a probability
  The first three come from ONE launch (as_disp_confidence).  A column holding a NaN or +inf is NaN in every map."""
  kinds = tuple(kinds)
  if not kinds or any(k not in KINDS for k in kinds) or len(set(kinds)) != len(kinds):
    raise ValueError("disparity_confidence: kinds %r must be a non-empty selection of %r without repeats" % (kinds, KINDS))
  logits = _check_volume(cost_volume)
  B, D, H, W = logits.shape
  out = {k: torch.empty(B, H, W, dtype=torch.float32, device=logits.device) for k in kinds}
  with torch.cuda.device(logits.device):
    if any(k != "fcs" for k in kinds):
      nat.call("as_disp_confidence", nat.ptr(logits), B, D, H, W, nat.ptr(out.get("pmax")), nat.ptr(out.get("entropy")),
               nat.ptr(out.get("mass")), nat.stream())
    if "fcs" in kinds:
      nat.call("as_fcs_scores", nat.ptr(logits), B, D, H, W, nat.ptr(out["fcs"]), None, None, 0, None, None, nat.stream())
  return out


def upsample_confidence(conf, H, W, out=None):
  """[B,1,H,W]: a confidence map [B,hc,wc] (or [B,1,hc,wc]) resized bilinearly, align_corners=False, values unscaled:
  as_upsample_bilinear_fwd with gain 1.  Never synchronises; allocates only when `out` is None."""
  nat.require_gpu(conf, out)
  shape = tuple(conf.shape)
  if conf.dim() == 4 and shape[1] == 1:
    shape = (shape[0],) + shape[2:]
  if len(shape) != 3 or min(shape) < 1 or conf.dtype != torch.float32 or not conf.is_contiguous():
    raise RuntimeError("upsample_confidence: expected a contiguous fp32 [B,hc,wc] or [B,1,hc,wc] tensor (got %s, %s, contiguous=%s)"
                       % (tuple(conf.shape), conf.dtype, conf.is_contiguous()))
  B, H, W = shape[0], int(H), int(W)
  if H < 1 or W < 1:
    raise ValueError("upsample_confidence: size %r x %r" % (H, W))
  if out is None:
    out = torch.empty(B, 1, H, W, dtype=torch.float32, device=conf.device)
  elif tuple(out.shape) != (B, 1, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != conf.device:
    raise RuntimeError("upsample_confidence: out must be a contiguous fp32 %s tensor on %s (got %s, %s, %s)"
                       % ((B, 1, H, W), conf.device, tuple(out.shape), out.dtype, out.device))
  with torch.cuda.device(conf.device):
    nat.call("as_upsample_bilinear_fwd", nat.ptr(conf.detach()), B, shape[1], shape[2], nat.ptr(out), H, W, 1.0, nat.stream())
  return out


def bin_scale(bins, lo, hi):
  """float32(bins / (hi - lo)), rounded once: the `scale` as_sparsification receives."""
  return float(np.float32(float(bins) / (float(hi) - float(lo))))


class SparsificationCollector(object):
  """Error statistics of a prediction against ground truth, binned by a key map (a confidence, or the error itself for the
  oracle): per bin the number of pixels with ground truth, the number whose error exceeds tau, and the fp64 sum of the absolute
  errors.  bin k = int((key - lo) * float32(bins / (hi - lo))), clamped to [0, bins - 1].  The buffers are allocated once."""

  def __init__(self, bins=256, lo=0.0, hi=1.0, tau=3.0, device="cuda"):
    self.bins, self.lo, self.hi, self.tau = int(bins), float(lo), float(hi), float(tau)
    if not (1 <= self.bins <= MAX_BINS):
      raise ValueError("SparsificationCollector: bins %r outside [1, %d]" % (bins, MAX_BINS))
    if not (np.isfinite(self.lo) and np.isfinite(self.hi) and self.hi > self.lo):
      raise ValueError("SparsificationCollector: need finite lo < hi (got %r, %r)" % (lo, hi))
    if self.tau != self.tau:
      raise ValueError("SparsificationCollector: tau is NaN")
    self.scale = bin_scale(self.bins, self.lo, self.hi)
    if not (np.isfinite(self.scale) and self.scale > 0):
      raise ValueError("SparsificationCollector: bins / (hi - lo) = %r is not a positive fp32 number" % (self.scale,))
    self.device = dev = gpu_device("SparsificationCollector", device)
    K = self.bins
    self._ints = torch.zeros(2 * K + 1, dtype=torch.int64, device=dev)        # count [K] | bad [K] | skipped
    self._err = torch.zeros(K, dtype=torch.float64, device=dev)

  def add(self, key, pred, gt):
    """Adds the elements of three contiguous fp32 tensors of one size (any shape).  Elements without ground truth (!(gt > 0)) are
    ignored; a NaN key or error is counted in counts()["skipped"].  Allocates nothing and never synchronises; inside a captured
    graph every replay adds."""
    n = key.numel()
    for name, t in (("key", key), ("pred", pred), ("gt", gt)):
      check_f32("SparsificationCollector.add", name, t, device=self._err.device, numel=n)
    if n < 1:
      raise RuntimeError("SparsificationCollector.add: empty input")
    K = self.bins
    with torch.cuda.device(self.device):
      nat.call("as_sparsification", nat.ptr(key), nat.ptr(pred), nat.ptr(gt), n, self.lo, self.scale, K, self.tau,
               nat.ptr(self._ints), nat.c_vp(self._ints.data_ptr() + 8 * K), nat.ptr(self._err),
               nat.c_vp(self._ints.data_ptr() + 16 * K), nat.stream())

  def counts(self):
    """Synchronises.  dict of numpy arrays: count, bad (int64 [bins]), abs_err (fp64 [bins]), and skipped as an int."""
    K = self.bins
    ints, err = self._ints.cpu().numpy(), self._err.cpu().numpy()
    return dict(count=ints[:K].copy(), bad=ints[K:2 * K].copy(), abs_err=err.copy(), skipped=int(ints[2 * K]))

  def reset(self):
    self._ints.zero_()
    self._err.zero_()

  def curve(self, remove="low"):
    """Synchronises.  sparsification_curve of counts()."""
    c = self.counts()
    return sparsification_curve(c["count"], c["bad"], c["abs_err"], remove)


def sparsification_curve(count, bad, abs_err, remove="low"):
  """(fraction_removed, epe_remaining, d1_remaining), each fp64 of length bins + 1: entry j is the state after the j bins with
  the lowest keys (remove="low": a confidence) or the highest keys (remove="high": an error) have been removed.  EPE and D1 are 0
  where nothing remains; the fractions are 0 when there is no pixel at all."""
  if remove not in ("low", "high"):
    raise ValueError("sparsification_curve: remove %r ('low' or 'high')" % (remove,))
  count, bad = np.asarray(count, dtype=np.float64), np.asarray(bad, dtype=np.float64)
  abs_err = np.asarray(abs_err, dtype=np.float64)
  if not (count.ndim == 1 and count.shape == bad.shape == abs_err.shape and count.size >= 1):
    raise ValueError("sparsification_curve: count %s, bad %s and abs_err %s must be 1-D and alike" % (count.shape, bad.shape, abs_err.shape))
  if remove == "high":
    count, bad, abs_err = count[::-1], bad[::-1], abs_err[::-1]

  def remaining(x):                                       # suffix sums: [sum of all, ..., last bin, 0]
    return np.concatenate([np.cumsum(x[::-1])[::-1], [0.0]])
  n, b, e = remaining(count), remaining(bad), remaining(abs_err)
  total = n[0]
  fraction = (total - n) / total if total > 0 else np.zeros_like(n)
  some = n > 0
  den = np.where(some, n, 1.0)
  return fraction, np.where(some, e / den, 0.0), np.where(some, b / den, 0.0)


def ause(curve, oracle_curve):
  """Area under the sparsification error: the trapezoid area between the EPE curve of a confidence and that of the oracle (a
  second collector keyed by |pred - gt|, curve("high")), each over its own fraction removed.  0 for a key that orders the
  pixels as their error does; the smaller, the better the confidence."""
  def area(c):
    x, y = np.asarray(c[0], dtype=np.float64), np.asarray(c[1], dtype=np.float64)
    if x.ndim != 1 or x.shape != y.shape or x.size < 2:
      raise ValueError("ause: a curve is (fraction_removed, epe_remaining, ...) of equal 1-D length >= 2")
    return float(np.sum((x[1:] - x[:-1]) * (y[1:] + y[:-1]) * 0.5))
  return area(curve) - area(oracle_curve)
