"""Edge-aware smoothing of a disparity map on the device (csrc/disp_smooth.hip): the image-guided weighted median, whose
uniform-weight case is the plain median.

consistency.py and disp_filter.py reject pixels and fill them from one row's background; this module repairs a map: it removes
the salt-and-pepper and the +-1 streaks a matcher's winner leaves, pulls blurred depth edges back onto the image's edges, and
fills a rejected pixel from its 2-D neighbourhood with respect for those edges.

  med = DisparitySmoother(H, W, batch=B, radius=1)                        # the plain 3 x 3 median
  sm = med(disp)                                                          # Smoothed: disp, code, counts
  wm = DisparitySmoother(H, W, batch=B, radius=3, sigma_color=0.1, fill=True, iterations=2)
  sm = wm(disp, guide=left, code_in=filt.code)                            # guided by the image, on what the filter kept

The output is always one of the input disparities (the lower median for equal weights and an even number of taps).  Codes are
those of disp_filter.CODE_NAMES: 0 wherever the result holds a kept or a filled value.  The contract is fixed op by op in
include/adaptive_stereo_hip.h.  There is no CPU path.
"""
import collections

import numpy as np
import torch

from . import _native as nat
from .collect import MapOperator, check_u8, int_in

COUNT_NAMES = ("unchanged", "changed", "filled", "rejected")
LUT_SIZE = 768
WEIGHT_ONE = 1024                       # the weight of a tap of the centre's own colour
MAX_RADIUS = 7

Smoothed = collections.namedtuple("Smoothed", "disp code counts")


class DisparitySmoother(MapOperator):
  """The weighted median for maps [batch,1,height,width] over a (2 * radius + 1)^2 window.  sigma_color None: every weight 1 (the
  plain median; a guide is refused).  Otherwise a tap's weight falls off with the sum over the channels of the absolute 8-bit
  colour difference k to the centre, exp(-k / (255 * channels * sigma_color)): sigma_color is in units of the image's range.
  fill: a pixel that is not usable takes the weighted median of its window when that holds at least min_support taps (default:
  half the window, rounded up).  iterations: passes, each on the previous one's result and code, so that fill grows into larger
  holes; counts are the last pass's.  All buffers are allocated once; a call enqueues only and is graph-capturable."""

  def __init__(self, height, width, batch=1, radius=2, sigma_color=None, channels=3, fill=False, min_support=None, iterations=1,
               device="cuda"):
    who = "DisparitySmoother"
    super().__init__(height, width, batch, device)
    if self.H * self.W > 2 ** 31 - 1 or self.B > 65535:
      raise ValueError("%s: %d x %d pixels (at most 2^31 - 1) in a batch of %d (at most 65535)" % (who, self.H, self.W, self.B))
    self.radius = int_in(who, "radius", radius, 1, MAX_RADIUS)
    if channels not in (1, 3):
      raise ValueError("%s: channels %r must be 1 or 3" % (who, channels))
    self.C = int(channels)
    self.sigma_color = None if sigma_color is None else float(sigma_color)
    if self.sigma_color is not None and not (0 < self.sigma_color < float("inf")):
      raise ValueError("%s: sigma_color %r must be a positive number (None: the plain median)" % (who, sigma_color))
    self.fill = bool(fill)
    taps = (2 * self.radius + 1) ** 2
    self.min_support = int_in(who, "min_support", (taps + 1) // 2 if min_support is None else min_support, 1, 2 ** 31 - 1)
    self.iterations = int_in(who, "iterations", iterations, 1, 8)
    self._table = None
    self._lut = None
    if self.sigma_color is not None:
      k = np.arange(LUT_SIZE, dtype=np.float64)
      w = np.maximum(1.0, np.round(WEIGHT_ONE * np.exp(-k / (255.0 * self.C * self.sigma_color))))
      self._table = np.where(k <= 255 * self.C, w, 0.0).astype(np.int32)
      self._lut = torch.from_numpy(self._table).to(self.device)
    shape = (self.B, 1, self.H, self.W)
    pairs = 1 if self.iterations == 1 else 2                                                  # later passes ping-pong
    self._out = [Smoothed(self._zeros(shape, torch.float32), self._zeros(shape, torch.uint8), None) for _ in range(pairs)]
    self._counts = self._zeros((self.B, len(COUNT_NAMES)), torch.int32)
    self._ran = False

  def weight_table(self):
    """int32 numpy [768]: the weight of a tap by its colour distance to the centre; all ones for the plain median."""
    return np.ones(LUT_SIZE, dtype=np.int32) if self._table is None else self._table.copy()

  def __call__(self, disp, guide=None, code_in=None):
    """Smoothed of views into this object's buffers: disp (fp32 [B,1,H,W]), code (uint8: 0 where disp holds a kept or a filled
    value, code_in or 4 elsewhere), counts (int32 [B,4]: COUNT_NAMES)."""
    who = "DisparitySmoother"
    self._check_map(who, "disp", disp)
    if code_in is not None:
      check_u8(who, "code_in", code_in, disp.shape, disp.device)
    if self._lut is None:
      if guide is not None:
        raise RuntimeError("%s: sigma_color None is the plain median and takes no guide" % who)
    else:
      if guide is None:
        raise RuntimeError("%s: sigma_color %g needs a guide [B,%d,H,W]" % (who, self.sigma_color, self.C))
      self._check_map(who, "guide", guide, self.C)
      guide = guide.detach()
    src, src_code = disp.detach(), code_in
    with torch.cuda.device(self.device):
      for it in range(self.iterations):
        dst = self._out[it % len(self._out)]
        last = it == self.iterations - 1
        nat.call("as_disp_wmedian", nat.ptr(src), nat.ptr(src_code), nat.ptr(guide), self.C, nat.ptr(self._lut), self.B, self.H,
                 self.W, self.radius, int(self.fill), self.min_support, nat.ptr(dst.disp), nat.ptr(dst.code),
                 nat.ptr(self._counts) if last else None, nat.stream())
        src, src_code = dst.disp, dst.code
    self._ran = True
    return dst._replace(counts=self._counts)

  def fractions(self):
    """Synchronises.  numpy fp64 [B,4]: the share of each of COUNT_NAMES per image in the last call's last pass."""
    if not self._ran:
      raise RuntimeError("DisparitySmoother.fractions: nothing has been smoothed yet")
    return self._fractions(self._counts)
