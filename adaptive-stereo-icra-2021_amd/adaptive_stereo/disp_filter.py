"""The post-filter of a disparity map before it becomes a point cloud (csrc/disp_filter.hip): the discontinuity (flying-pixel)
check and the speckle filter, on the device, chained with the left-right check and the fill of adaptive_stereo.consistency.

confidence.py answers "how sure is the network", consistency.py "does the other view agree"; this module answers "is this pixel
geometrically isolated": it sits on the ramp the refinement blurs a depth edge into, or in a small island of disparity nothing
around it shares.

  flt = DisparityFilter(H, W, batch=B, tol_abs=1.0, max_diff=1.0, max_size=200)
  filt = flt(disp)                                      # DispFilter: code, valid, jump, label, size, counts
  filt = flt(disp, code_in=chk.code_l)                  # on what the left-right check kept
  cloud = proj.voxel_cloud(disp, left, confidence=filt.valid, conf_min=1.0)    # pointcloud.DepthProjector
  filled = lrc.fill(disp, filt.code)                    # as_lr_fill takes every non-zero code as "fill me"

  both = FilteredBothViewInference(feature_net, stereo_net, H, W, batch=B).capture()    # one hipGraph replay
  disp_l, disp_r, chk, filt, filled_l = both(left, right)

Codes extend consistency.CODE_NAMES: 5 discontinuity, 6 speckle.  The two contracts are fixed op by op in
include/adaptive_stereo_hip.h.  There is no CPU path.
"""
import collections

import torch

from . import _native as nat
from . import consistency
from .collect import MapOperator, check_u8, int_in

CODE_NAMES = consistency.CODE_NAMES + ("discontinuity", "speckle")

DispFilter = collections.namedtuple("DispFilter", "code valid jump label size counts")


class DisparityFilter(MapOperator):
  """The edge check and the speckle pass for maps [batch,1,height,width].  All output buffers are allocated once; every call
  overwrites them, enqueues only and is graph-capturable.  An edge is |d - neighbour| > max(tol_abs, tol_rel * d) against a usable
  4-neighbour; a speckle is a 4-connected component of at most max_size pixels, neighbours being joined when they differ by at
  most max_diff (+inf: every usable pair)."""

  def __init__(self, height, width, batch=1, tol_abs=1.0, tol_rel=0.0, max_diff=1.0, max_size=200, device="cuda"):
    super().__init__(height, width, batch, device)
    if self.H * self.W > 2 ** 31 - 1 or self.B > 65535:
      raise ValueError("DisparityFilter: %d x %d pixels (at most 2^31 - 1) in a batch of %d (at most 65535)" % (self.H, self.W, self.B))
    self.tol_abs, self.tol_rel, self.max_diff = float(tol_abs), float(tol_rel), float(max_diff)
    if not (self.tol_abs >= 0 and self.tol_rel >= 0):
      raise ValueError("DisparityFilter: tol_abs %r and tol_rel %r must be numbers and not negative" % (tol_abs, tol_rel))
    if not self.max_diff >= 0:
      raise ValueError("DisparityFilter: max_diff %r must be a number and not negative" % (max_diff,))
    self.max_size = int_in("DisparityFilter", "max_size", max_size, 0, 2 ** 31 - 1)
    shape = (self.B, 1, self.H, self.W)
    u8 = lambda: self._zeros(shape, torch.uint8)
    f32 = lambda: self._zeros(shape, torch.float32)
    i32 = lambda: self._zeros(shape, torch.int32)
    counts = lambda: self._zeros((self.B, len(CODE_NAMES)), torch.int32)
    self._edges = DispFilter(u8(), f32(), f32(), None, None, counts())            # the speckle pass reads the edge pass's code
    self._speckles = DispFilter(u8(), f32(), None, i32(), i32(), counts())
    self._both = self._speckles._replace(jump=self._edges.jump)
    self._last = None

  def _check_maps(self, who, disp, code_in):
    self._check_map(who, "disp", disp)
    if code_in is not None:
      check_u8(who, "code_in", code_in, disp.shape, disp.device)

  def edges(self, disp, code_in=None):
    """DispFilter of views into this object's buffers: code (uint8: code_in where non-zero, 4 bad input, 5 discontinuity, else
    0), valid (fp32 1.0 / 0.0), jump (the largest difference to a usable 4-neighbour; NaN where the pixel itself is not
    usable), counts (int32 [B,7]); label and size are None."""
    self._check_maps("DisparityFilter.edges", disp, code_in)
    r = self._edges
    with torch.cuda.device(self.device):
      nat.call("as_disp_edge_check", nat.ptr(disp.detach()), nat.ptr(code_in), self.B, self.H, self.W, self.tol_abs, self.tol_rel,
               nat.ptr(r.code), nat.ptr(r.valid), nat.ptr(r.jump), nat.ptr(r.counts), nat.stream())
    self._last = r
    return r

  def speckles(self, disp, code_in=None):
    """DispFilter: label (int32: the smallest index y * W + x of the pixel's component, -1 where not usable), size (int32: the
    component's pixels, 0 where not usable), code (code_in where non-zero, 4 bad input, 6 where size <= max_size, else 0), valid,
    counts; jump is None."""
    self._check_maps("DisparityFilter.speckles", disp, code_in)
    return self._run_speckles(disp, code_in, self._speckles)

  def _run_speckles(self, disp, code_in, r):
    with torch.cuda.device(self.device):
      nat.call("as_disp_speckle", nat.ptr(disp.detach()), nat.ptr(code_in), self.B, self.H, self.W, self.max_diff, self.max_size,
               nat.ptr(r.label), nat.ptr(r.size), nat.ptr(r.code), nat.ptr(r.valid), nat.ptr(r.counts), nat.stream())
    self._last = r
    return r

  def __call__(self, disp, code_in=None):
    """edges(), then speckles() on what the edges kept: one DispFilter whose code, valid and counts are the final ones (codes of
    code_in, 4, 5 and 6 together), jump the edge pass's, label and size the components of the pixels that passed it."""
    self._check_maps("DisparityFilter", disp, code_in)
    e = self.edges(disp, code_in)
    return self._run_speckles(disp, e.code, self._both)

  def fractions(self):
    """Synchronises.  numpy fp64 [B,7]: the share of each code per image in the last call."""
    if self._last is None:
      raise RuntimeError("DisparityFilter.fractions: nothing has been filtered yet")
    return self._fractions(self._last.counts)


class FilteredBothViewInference(consistency.BothViewInference):
  """BothViewInference with the post-filter in the chain: mirror, one forward pass over both views, the left-right check, the
  filter of the left view on what the check kept, the flip back, and the fill of the left view from the COMBINED code (rejected
  by the check, discontinuity or speckle).  ``__call__(left, right)`` -> (disp_l, disp_r, LRCheck, DispFilter, filled_l); after
  capture() one graph replay.

  smooth_radius > 0 adds the weighted median of smooth.DisparitySmoother at the end of the chain (off by default: the chain and
  its result are then what they were): on the left view, on what the filter kept (code_in = DispFilter.code), guided by the left
  image when smooth_sigma is given (the plain median otherwise), filling rejected pixels with smooth_fill.  The result gains a
  sixth element, its Smoothed; filled_l stays the row fill of the unsmoothed map."""

  def __init__(self, feature_net, stereo_net, height, width, batch=1, tol_abs=1.0, tol_rel=0.0, channels=3, edge_tol_abs=1.0,
               edge_tol_rel=0.0, max_diff=1.0, max_size=200, smooth_radius=0, smooth_sigma=None, smooth_fill=False):
    super().__init__(feature_net, stereo_net, height, width, batch, tol_abs, tol_rel, channels)
    self.filter = DisparityFilter(height, width, batch, edge_tol_abs, edge_tol_rel, max_diff, max_size, device=self.lrc.device)
    self.smoother = None
    if smooth_radius:
      from .smooth import DisparitySmoother
      self.smoother = DisparitySmoother(height, width, batch, radius=smooth_radius, sigma_color=smooth_sigma, channels=channels,
                                        fill=smooth_fill, device=self.lrc.device)

  def _eager(self, left, right):
    disp_l, mirrored_r, chk = self._forward_and_check(left, right)
    filt = self.filter(disp_l, chk.code_l)
    consistency.flip_w(mirrored_r, out=self._disp_r)
    result = disp_l, self._disp_r, chk, filt, self.lrc.fill(disp_l, filt.code)
    if self.smoother is None:
      return result
    guide = left if self.smoother.sigma_color is not None else None
    return result + (self.smoother(disp_l, guide, filt.code),)
