"""Calibrating the OOD gate: per-image feature-contrast scores on the device, the threshold, and the evidence that it separates
two domains (csrc/ood.hip).

What the reference's evaluation/ood_analysis.py computes: it runs the training domain through the network in eval mode, keeps
``feature_contrast_mean(cost_volume).mean(dim=(-2, -1))`` per image (:76-77, read back per batch), fits a normal distribution
and takes a low percentile as ``--ood_threshold`` (:203-205); against a novel domain it sweeps 100 cutoffs for a precision/recall
curve (:107-127, four ``.item()`` per cutoff) and draws both histograms over shared bins (:196-199).  Here the scores of a batch
are one launch appended at a device-side cursor, the sweep is one broadcast compare with one read-back, and the plots are left
to the caller: every function returns the numbers a plot would show.

  collector = FcsCollector(1000)
  collector.add(outputs["cost_volume_l/4"])              # no allocation, no synchronisation: graph-capturable
  train = collector.scores()[:, 0]                        # synchronises; column 0 max-minus-mean, column 1 max-minus-median
  threshold, mu, sigma = ood_threshold(train, 0.05)       # --ood_threshold
"""
import contextlib
import math
import statistics

import numpy as np
import torch

from . import _native as nat
from .collect import RowCursor, check_f32, eval_batches


def _logits(cost_volume):
  nat.require_gpu(cost_volume)
  logits = nat.f32c(cost_volume.detach())
  if logits.dim() != 4:
    raise RuntimeError("adaptive_stereo.ood: cost_volume has shape %s, expected [B,D,H,W]" % (tuple(logits.shape),))
  return logits


def fcs_scores(cost_volume, maps=False):
  """scores [B,2] of a logits volume [B,D,H,W]: per image the mean over H x W of the max-minus-mean map (column 0) and of the
  max-minus-median map (column 1).  With maps=True: (scores, fcs_mean [B,H,W], fcs_median [B,H,W]).  Never synchronises.
  The mean map is as_softargmax_fwd's fcs bit for bit; the by-product StereoNet attaches to its logits (what
  feature_contrast_mean returns for them) comes from the fused tail kernel, which adds the D values in another order and
  differs from it in the last bits."""
  with torch.no_grad():
    logits = _logits(cost_volume)
    B, D, H, W = logits.shape
    scores = torch.empty(B, 2, dtype=torch.float32, device=logits.device)
    fmean = torch.empty(B, H, W, dtype=torch.float32, device=logits.device) if maps else None
    fmed = torch.empty_like(fmean) if maps else None
    with torch.cuda.device(logits.device):
      nat.call("as_fcs_scores", nat.ptr(logits), B, D, H, W, nat.ptr(fmean), nat.ptr(fmed), nat.ptr(scores), B, None, None,
               nat.stream())
  return (scores, fmean, fmed) if maps else scores


class FcsCollector(RowCursor):
  """A [capacity,2] score buffer on the device with its cursor and a counter of the rows that did not fit, allocated once."""

  def __init__(self, capacity, device="cuda"):
    super().__init__("FcsCollector", capacity, device)
    self._scores = torch.zeros(self.capacity, 2, dtype=torch.float32, device=self.device)

  def add(self, cost_volume):
    """Appends the B rows of a contiguous fp32 volume [B,D,H,W] at the cursor.  Allocates nothing and never synchronises; inside
    a captured graph every replay appends.  Rows beyond the capacity are counted in dropped()."""
    check_f32("FcsCollector.add", "cost_volume", cost_volume, ((4,), "[B,D,H,W]"), self._scores.device)
    B, D, H, W = cost_volume.shape
    with torch.cuda.device(self.device):
      nat.call("as_fcs_scores", nat.ptr(cost_volume), B, D, H, W, None, None, nat.ptr(self._scores), self.capacity,
               nat.ptr(self._cursor), nat.ptr(self._dropped), nat.stream())

  def scores(self):
    """Synchronises.  The rows in use, [n,2] (a clone: later add() calls do not change it)."""
    return self._scores[:self.rows_in_use()].clone()


def collect_scores(feature_net, stereo_net, batches, num_images, input_scale=0):
  """Scores [n,2] (n <= num_images) of the left cost volume over `batches`, any iterable of dicts with ``color_l/{s}`` and
  ``color_r/{s}``: collect.eval_batches (eval mode, no_grad, forward with output_cost_volume=True), FcsCollector.add (the
  compute of the reference's save_data, ood_analysis.py:40-90).  Stops once num_images rows are in; one read-back, at the end.
  Each network's train/eval state is restored."""
  key = "cost_volume_l/{}".format(int(input_scale) + stereo_net.k)
  collector = None
  with torch.no_grad(), contextlib.closing(eval_batches(feature_net, stereo_net, batches, num_images, input_scale)) as passes:
    for _, _, left, outputs in passes:
      if collector is None:
        collector = FcsCollector(num_images, device=left.device)
      collector.add(nat.f32c(outputs[key].detach()))
  if collector is None:
    return torch.zeros(0, 2, dtype=torch.float32)
  return collector.scores()


def collect_image_entropy(batches, num_images, input_scale=0):
  """Scores [n,2] (n <= num_images) of the left image over `batches`, any iterable of dicts with ``color_l/{s}``: column 0 the
  entropy of the 8-bit intensities, column 1 that of their horizontal differences (utils/entropy.py: EntropyCollector.add per
  batch).  No network pass.  Stops once num_images rows are in; one read-back, at the end."""
  from .utils.entropy import EntropyCollector
  key = "color_l/{}".format(int(input_scale))
  collector, seen = None, 0
  for inputs in batches:
    if seen >= num_images:
      break
    left = nat.f32c(inputs[key].cuda())
    if collector is None:
      collector = EntropyCollector(num_images, device=left.device)
    collector.add(left)
    seen += left.shape[0]
  if collector is None:
    return torch.zeros(0, 2, dtype=torch.float32)
  return collector.scores()


def _as_f32_1d(scores, name):
  t = torch.as_tensor(scores).detach()
  if t.dim() != 1 or t.numel() == 0:
    raise ValueError("adaptive_stereo.ood: %s must be a non-empty 1-D set of scores (got shape %s)" % (name, tuple(t.shape)))
  return t.to(torch.float32)


def ood_threshold(train_scores, percentile):
  """(threshold, mu, sigma): mu + sigma * inverse-normal-cdf(percentile) in fp64, mu the mean and sigma the square root of the
  unbiased variance of the training domain's scores (ood_analysis.py:203-204).  One score has no variance: sigma is NaN."""
  if not (0.01 <= percentile <= 0.99):
    raise ValueError("ood_threshold: percentile %r outside [0.01, 0.99]" % (percentile,))
  x = _as_f32_1d(train_scores, "train_scores").cpu().numpy().astype(np.float64)
  mu = float(x.mean())
  sigma = math.sqrt(float(x.var(ddof=1))) if x.size > 1 else float("nan")
  z = statistics.NormalDist().inv_cdf(float(percentile))
  return mu + sigma * z, mu, sigma


def precision_recall(train_scores, novel_scores, num=100):
  """Sweep of `num` cutoffs np.linspace(novel.min(), novel.max(), num), each rounded to fp32 (torch compares an fp32 tensor with
  a Python scalar in fp32); an example is called novel when its score is <= the cutoff (ood_analysis.py:93-120).  Returns a dict
  of numpy arrays: cutoffs (fp32), tp, fn, tn, fp (int64), precision (1.0 where tp + fp == 0) and recall (fp64).  The counts are
  one broadcast compare-and-sum on the scores' device (the novel set's when the two differ) and one read-back."""
  train, novel = _as_f32_1d(train_scores, "train_scores"), _as_f32_1d(novel_scores, "novel_scores")
  num = int(num)
  if num < 1:
    raise ValueError("precision_recall: num %r must be at least 1" % (num,))
  if train.device != novel.device:
    train = train.to(novel.device)
  # np.linspace's own fp64 operations, one at a time, where the scores are: arange * step + start, the last one set to stop
  lo, hi = novel.min().double(), novel.max().double()
  c64 = torch.arange(num, dtype=torch.float64, device=novel.device) * ((hi - lo) / max(num - 1, 1)) + lo
  if num > 1:
    c64[-1] = hi
  c = c64.float()[:, None]
  back = torch.stack([c[:, 0].double(), (novel[None, :] <= c).sum(dim=1).double(),
                      (train[None, :] <= c).sum(dim=1).double()]).cpu().numpy()      # counts are exact in fp64
  cutoffs, tp, fp = back[0].astype(np.float32), back[1].astype(np.int64), back[2].astype(np.int64)
  fn, tn = novel.numel() - tp, train.numel() - fp
  called = tp + fp
  precision = np.where(called > 0, tp / np.maximum(called, 1).astype(np.float64), 1.0)
  recall = tp / float(novel.numel())
  return dict(cutoffs=cutoffs, tp=tp, fn=fn, tn=tn, fp=fp, precision=precision, recall=recall)


def strictly_decreasing_precision(pr, re):
  """(recall ascending, precision): every precision replaced by the highest one at its recall or beyond, so the curve never
  rises with recall (ood_analysis.py:146-161)."""
  pr, re = np.asarray(pr, dtype=np.float64), np.asarray(re, dtype=np.float64)
  if pr.shape != re.shape or pr.ndim != 1:
    raise ValueError("strictly_decreasing_precision: pr %s and re %s must be 1-D and alike" % (pr.shape, re.shape))
  order = np.argsort(re)
  re_desc, pr_desc = re[order][::-1], pr[order][::-1]
  return re_desc[::-1].copy(), np.maximum.accumulate(pr_desc)[::-1].copy()


def fcs_histogram(train_scores, novel_scores, bins=40):
  """(edges [bins + 1], train density [bins], novel density [bins]): equal-width bins over both sets together, each set's
  histogram normalised to unit area (ood_analysis.py:196-199)."""
  t = _as_f32_1d(train_scores, "train_scores").cpu().numpy()
  n = _as_f32_1d(novel_scores, "novel_scores").cpu().numpy()
  edges = np.histogram(np.hstack((t, n)), bins=bins)[1]
  return edges, np.histogram(t, edges, density=True)[0], np.histogram(n, edges, density=True)[0]
