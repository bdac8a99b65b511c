"""Probing a cost volume where its feature-contrast score is extreme: per image the pixel with the largest and the one with the
smallest max-minus-mean value, their matching curves over disparity, and the mean per rank of every pixel's sorted logits
(csrc/cv_probe.hip).

What the reference's evaluation/cost_volume_analysis.py computes per image on the host: feature_contrast_mean, torch.argmax
(train domain) or torch.argmin (novel domain) of the flattened map, the slice there, torch.sort, sorted[0], sorted[2:].mean() and
the true disparity (:82-92).  Here that is one launch per batch appended at a device-side cursor; the pick is taken on the map
the OOD gate itself uses (as_fcs_scores' mean map, bit for bit).

  probe = CostVolumeProbe(10, D=12, profile=True)
  probe.add(outputs["cost_volume_l/4"], inputs["gt_disp_l/4"])     # no allocation, no synchronisation: graph-capturable
  res = probe.results()                                              # synchronises
  res.slices[i, HI], res.max[i, HI], res.mean_rest[i, HI], res.gt[i, HI]     # what the reference's figure shows for image i

Rules: an image holding a NaN selects its first NaN pixel both times (d_max -1, max / mean_rest NaN, profile all NaN); for D <= 2
the map is 0 everywhere, so both picks are pixel 0 and mean_rest is NaN.
"""
import contextlib

import torch

from . import _native as nat
from .collect import RowCursor, check_f32, eval_batches

HI, LO = 0, 1          # index of the second axis: the pixel where the map is largest / smallest


class ProbeResult(object):
  """Device tensors of n probed images: pix [n,2,3] int32 (row, col, d_max), vals [n,2,5] fp32 (fcs, max, second, mean_rest, gt),
  slices [n,2,D] fp32, profile [n,D] fp32 or None.  The second axis is (HI, LO).  The named views share their memory."""

  def __init__(self, pix, vals, slices, profile=None):
    self.pix, self.vals, self.slices, self.profile = pix, vals, slices, profile

  row = property(lambda self: self.pix[..., 0])
  col = property(lambda self: self.pix[..., 1])
  d_max = property(lambda self: self.pix[..., 2])
  fcs = property(lambda self: self.vals[..., 0])
  max = property(lambda self: self.vals[..., 1])
  second = property(lambda self: self.vals[..., 2])
  mean_rest = property(lambda self: self.vals[..., 3])
  gt = property(lambda self: self.vals[..., 4])

  def __len__(self):
    return self.pix.shape[0]

  def cpu(self):
    return ProbeResult(self.pix.cpu(), self.vals.cpu(), self.slices.cpu(), None if self.profile is None else self.profile.cpu())

  def state_dict(self):
    out = dict(pix=self.pix, vals=self.vals, slices=self.slices)
    if self.profile is not None:
      out["profile"] = self.profile
    return out


def _check_gt(gt, cost_volume, who):
  if gt is None:
    return
  B, D, H, W = cost_volume.shape
  if gt.dtype != torch.float32 or not gt.is_contiguous() or gt.device != cost_volume.device or \
     tuple(gt.shape) not in ((B, 1, H, W), (B, H, W)):
    raise RuntimeError("%s: gt must be a contiguous fp32 [B,1,H,W] tensor beside the volume %s on %s (got %s, %s, %s, "
                       "contiguous=%s)" % (who, tuple(cost_volume.shape), cost_volume.device, tuple(gt.shape), gt.dtype,
                                           gt.device, gt.is_contiguous()))


def probe_cost_volume(cost_volume, gt=None, profile=False):
  """ProbeResult of a logits volume [B,D,H,W] (and the coarse ground truth [B,1,H,W], if given).  Never synchronises."""
  with torch.no_grad():
    nat.require_gpu(cost_volume, gt)
    logits = nat.f32c(cost_volume.detach())
    if logits.dim() != 4:
      raise RuntimeError("adaptive_stereo.cv_probe: cost_volume has shape %s, expected [B,D,H,W]" % (tuple(logits.shape),))
    gt = nat.f32c(gt.detach()) if gt is not None else None
    _check_gt(gt, logits, "probe_cost_volume")
    B, D, H, W = logits.shape
    dev = logits.device
    pix = torch.empty(B, 2, 3, dtype=torch.int32, device=dev)
    vals = torch.empty(B, 2, 5, dtype=torch.float32, device=dev)
    slices = torch.empty(B, 2, D, dtype=torch.float32, device=dev)
    prof = torch.empty(B, D, dtype=torch.float32, device=dev) if profile else None
    with torch.cuda.device(dev):
      nat.call("as_cost_volume_probe", nat.ptr(logits), nat.ptr(gt), B, D, H, W, nat.ptr(pix), nat.ptr(vals), nat.ptr(slices),
               nat.ptr(prof), B, None, None, nat.stream())
  return ProbeResult(pix, vals, slices, prof)


class CostVolumeProbe(RowCursor):
  """Row buffers for `capacity` images of D disparities on the device, with their cursor and a counter of the rows that did not
  fit, allocated once."""

  def __init__(self, capacity, D, profile=False, device="cuda"):
    self.D = int(D)
    if not (1 <= self.D <= 64):
      raise ValueError("CostVolumeProbe: D %r outside [1, 64]" % (D,))
    super().__init__("CostVolumeProbe", capacity, device)
    dev = self.device
    self._pix = torch.zeros(self.capacity, 2, 3, dtype=torch.int32, device=dev)
    self._vals = torch.zeros(self.capacity, 2, 5, dtype=torch.float32, device=dev)
    self._slices = torch.zeros(self.capacity, 2, self.D, dtype=torch.float32, device=dev)
    self._profile = torch.zeros(self.capacity, self.D, dtype=torch.float32, device=dev) if profile else None

  def add(self, cost_volume, gt=None):
    """Appends the B rows of a contiguous fp32 volume [B,D,H,W] at the cursor.  Allocates nothing and never synchronises; inside
    a captured graph every replay appends.  Rows beyond the capacity are counted in dropped()."""
    check_f32("CostVolumeProbe.add", "cost_volume", cost_volume, ((4,), "[B,D,H,W]"), self._pix.device)
    nat.require_gpu(gt)
    B, D, H, W = cost_volume.shape
    if D != self.D:
      raise RuntimeError("CostVolumeProbe.add: the volume has D %d, the buffers were allocated for D %d" % (D, self.D))
    _check_gt(gt, cost_volume, "CostVolumeProbe.add")
    with torch.cuda.device(self.device):
      nat.call("as_cost_volume_probe", nat.ptr(cost_volume), nat.ptr(gt), B, D, H, W, nat.ptr(self._pix), nat.ptr(self._vals),
               nat.ptr(self._slices), nat.ptr(self._profile), self.capacity, nat.ptr(self._cursor), nat.ptr(self._dropped),
               nat.stream())

  def results(self):
    """Synchronises.  The rows in use as a ProbeResult (clones: later add() calls do not change them)."""
    n = self.rows_in_use()
    return ProbeResult(self._pix[:n].clone(), self._vals[:n].clone(), self._slices[:n].clone(),
                       None if self._profile is None else self._profile[:n].clone())


def collect_probes(feature_net, stereo_net, batches, num_images, input_scale=0, profile=False, on_batch=None):
  """ProbeResult of n <= num_images images of the left cost volume over `batches`, any iterable of dicts with ``color_l/{s}``,
  ``color_r/{s}`` and, when it is there, ``gt_disp_l/{s+k}``: collect.eval_batches (eval mode, no_grad, forward with
  output_cost_volume=True), CostVolumeProbe.add (the compute of the reference's save_cost_volumes and of the numbers in
  visualize_cost_volumes, cost_volume_analysis.py:34-92).  Stops once num_images rows are in; one read-back, at the end.  Each
  network's train/eval state is restored.  ``on_batch(first_index, cost_volume, gt)`` is called per batch with the device
  tensors (gt may be None)."""
  key = "cost_volume_l/{}".format(int(input_scale) + stereo_net.k)
  gt_key = "gt_disp_l/{}".format(int(input_scale) + stereo_net.k)
  probe = None
  with torch.no_grad(), contextlib.closing(eval_batches(feature_net, stereo_net, batches, num_images, input_scale)) as passes:
    for first, inputs, _, outputs in passes:
      logits = nat.f32c(outputs[key].detach())
      gt = nat.f32c(inputs[gt_key].cuda()) if gt_key in inputs else None
      if gt is not None and gt.dim() == 3:
        gt = gt.unsqueeze(1)
      if probe is None:
        probe = CostVolumeProbe(num_images, logits.shape[1], profile=profile, device=logits.device)
      probe.add(logits, gt)
      if on_batch is not None:
        on_batch(first, logits, gt)
  if probe is None:
    return ProbeResult(torch.zeros(0, 2, 3, dtype=torch.int32), torch.zeros(0, 2, 5), torch.zeros(0, 2, 0),
                       torch.zeros(0, 0) if profile else None)
  return probe.results()
