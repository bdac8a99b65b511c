"""Feature-contrast score (OOD score) — reference adaptive_stereo/utils/feature_contrast.py:12-23.

The reference sorts the whole [B,Dc,Hc,Wc] volume along Dc to take ``max - mean(sorted[2:])``.
Only the two largest values and the sum are needed: fcs = m1 - (sum - m1 - m2)/(Dc-2), which the
soft-argmax kernel already produces in the same pass over the logits.  StereoNet.forward attaches
that by-product to the logits tensor together with the tensor's version counter; a volume that did not
come from StereoNet — or one a caller has edited in place since (the counter moved) — is scored by running
the kernel on it, as the reference recomputes on every call.

feature_contrast_median (reference :4-9, ``max - torch.median`` along Dc: the lower median) has no by-product to reuse: it is
one launch of as_fcs_scores (csrc/ood.hip) with only the median map requested.
"""
import torch

from .. import _native as nat


def feature_contrast_mean(cost_volume):
  nat.require_gpu(cost_volume)
  cached = getattr(cost_volume, "_as_fcs", None)
  if cached is not None and getattr(cost_volume, "_as_fcs_version", None) == cost_volume._version:
    return cached
  with torch.no_grad():
    logits = nat.f32c(cost_volume.detach())
    B, D, H, W = logits.shape
    pred = torch.empty(B, H, W, dtype=torch.float32, device=logits.device)
    fcs = torch.empty_like(pred)
    nat.call("as_softargmax_fwd", nat.ptr(logits), B, D, H, W, nat.ptr(pred), None, nat.ptr(fcs), nat.stream())
    return fcs


def feature_contrast_median(cost_volume):
  nat.require_gpu(cost_volume)
  with torch.no_grad():
    logits = nat.f32c(cost_volume.detach())
    B, D, H, W = logits.shape
    fcs = torch.empty(B, H, W, dtype=torch.float32, device=logits.device)
    with torch.cuda.device(logits.device):
      nat.call("as_fcs_scores", nat.ptr(logits), B, D, H, W, None, nat.ptr(fcs), None, 0, None, None, nat.stream())
    return fcs
