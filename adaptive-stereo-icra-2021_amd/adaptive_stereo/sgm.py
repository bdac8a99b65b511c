"""Semi-global matching on the device (csrc/sgm.hip): a second, network-independent source of disparity.

The network answers "what does the model see"; this module answers "what does a classical matcher see in the same pair": a 9 x 7
census transform, Hamming costs, 4 or 8 aggregation paths, winner selection with a uniqueness test and a sub-pixel parabola, for
the left and the right view out of one volume.  It serves two purposes: a baseline to put beside the network's figures
(sgm_baseline.py), and sparse proxy labels for the supervised step where ground truth is missing.

  sgm = SemiGlobalMatcher(H, W, batch=B, maxdisp=192)
  res = sgm(left, right)                                # SGMResult: disp_l, disp_r, code_l, code_r, counts
  res = sgm(left, right, fill=0.0)                      # 0.0 where rejected: "no label" to the loss and the metrics

  lab = ProxyLabeler(H, W, batch=B).capture()           # matcher, left-right check, speckle filter: one hipGraph replay
  labels, code, counts = lab(left, right)               # labels: disp_l where every stage kept the pixel, 0.0 elsewhere
  losses = proxy_supervised_step(trainer, lab, left, right)                   # training.SupervisedTrainer

``fill``: NaN in front of LeftRightConsistency.check, whose first step turns it into code 4; 0.0 in front of the supervised loss
and the metrics, which read gt <= 0 as "no label".  Codes extend disp_filter.CODE_NAMES by 7, not unique.  The four contracts
are fixed op by op in include/adaptive_stereo_hip.h.  There is no CPU path.
"""
import collections

import torch

from . import _native as nat
from . import disp_filter
from . import smooth
from .capture import copy_unless_same, refuse_nested, warm_up_and_capture
from .collect import MapOperator, check_f32, int_in
from .consistency import LeftRightConsistency

CODE_NAMES = disp_filter.CODE_NAMES + ("not_unique",)

SGMResult = collections.namedtuple("SGMResult", "disp_l disp_r code_l code_r counts")


class SemiGlobalMatcher(MapOperator):
  """Census, aggregation and selection for pairs [batch,channels,height,width].  All buffers, the aggregation volume included
  (2 * batch * height * width * maxdisp bytes), are allocated once; every call overwrites them, enqueues only and is
  graph-capturable.  p1, p2: the penalties of a disparity step of one and of more than one along a path; uniqueness: the margin in
  per cent by which the winner must undercut every disparity that is not its neighbour.  The defaults (p1 10, p2 120, 8 paths,
  uniqueness 5) are the values customary for 9 x 7 census costs; they are NOT tuned here."""

  def __init__(self, height, width, batch=1, maxdisp=192, p1=10, p2=120, paths=8, uniqueness=5, channels=3, device="cuda"):
    who = "SemiGlobalMatcher"
    super().__init__(height, width, batch, device)
    self.D = int_in(who, "maxdisp", maxdisp, 1, 256)
    if self.H * self.W * self.D > 2 ** 31 - 1 or self.B > 65535:
      raise ValueError("%s: %d x %d pixels x %d disparities (at most 2^31 - 1) in a batch of %d (at most 65535)"
                       % (who, self.H, self.W, self.D, self.B))
    self.p1 = int_in(who, "p1", p1, 0, 255)
    self.p2 = int_in(who, "p2", p2, self.p1, 255)
    if paths not in (4, 8):
      raise ValueError("%s: paths %r must be 4 or 8" % (who, paths))
    self.paths = int(paths)
    self.uniqueness = int_in(who, "uniqueness", uniqueness, 0, 99)
    if channels not in (1, 3):
      raise ValueError("%s: channels %r must be 1 or 3" % (who, channels))
    self.C = int(channels)
    shape = (self.B, 1, self.H, self.W)
    self._census = self._zeros((2, self.B, self.H, self.W), torch.int64)                          # left, right: uint64 words
    nbytes = nat.load().as_sgm_workspace(self.B, self.H, self.W, self.D)
    if nbytes <= 0:
      raise RuntimeError("%s: as_sgm_workspace refused %d x %d x %d x %d" % (who, self.B, self.H, self.W, self.D))
    self._volume = self._zeros(nbytes // 2, torch.int16)                                          # uint16 [B][H][W][D]
    f32 = lambda: self._zeros(shape, torch.float32)
    u8 = lambda: self._zeros(shape, torch.uint8)
    self._result = SGMResult(f32(), f32(), u8(), u8(), self._zeros((self.B, 2, len(CODE_NAMES)), torch.int32))
    self._ran = False

  def _check_image(self, who, name, img):
    self._check_map(who, name, img, self.C)

  def _census_into(self, img, out):
    with torch.cuda.device(self.device):
      nat.call("as_sgm_census", nat.ptr(img.detach()), self.B, self.C, self.H, self.W, nat.ptr(out), nat.stream())
    return out

  def census(self, img, right=False):
    """The census words of one image: int64 [B,H,W] holding the uint64 bit patterns, a view of this object's buffer for the left
    (or, right=True, the right) view."""
    self._check_image("SemiGlobalMatcher.census", "img", img)
    return self._census_into(img, self._census[1 if right else 0])

  def volume(self):
    """The aggregation volume S of the last call: int16 [B,H,W,D] holding uint16 sums (at most 2552, so the sign never shows)."""
    return self._volume.view(self.B, self.H, self.W, self.D)

  def __call__(self, left, right, fill=float("nan")):
    who = "SemiGlobalMatcher"
    self._check_image(who, "left", left)
    self._check_image(who, "right", right)
    r = self._result
    self._census_into(left, self._census[0])
    self._census_into(right, self._census[1])
    with torch.cuda.device(self.device):
      nat.call("as_sgm_aggregate", nat.ptr(self._census[0]), nat.ptr(self._census[1]), self.B, self.H, self.W, self.D, self.p1,
               self.p2, self.paths, nat.ptr(self._volume), nat.stream())
      nat.call("as_sgm_select", nat.ptr(self._volume), self.B, self.H, self.W, self.D, self.uniqueness, float(fill),
               nat.ptr(r.disp_l), nat.ptr(r.code_l), nat.ptr(r.disp_r), nat.ptr(r.code_r), nat.ptr(r.counts), nat.stream())
    self._ran = True
    return r

  def result(self):
    """The SGMResult of views into this object's buffers, as the last call left them."""
    return self._result

  def fractions(self):
    """Synchronises.  numpy fp64 [B,2,8]: the share of each code per image and view in the last call."""
    if not self._ran:
      raise RuntimeError("SemiGlobalMatcher.fractions: nothing has been matched yet")
    return self._fractions(self._result.counts)


class ProxyLabeler(object):
  """Sparse proxy labels from the matcher: SemiGlobalMatcher (fill NaN), with median_radius > 0 the plain median of its two views
  (smooth.DisparitySmoother; disp_l is then the smoothed map), LeftRightConsistency.check of the two views,
  DisparityFilter.speckles on what the check kept, labels = disp_l where the final code is 0 and 0.0 elsewhere.
  ``__call__(left, right)`` -> (labels [B,1,H,W], code uint8 [B,1,H,W], counts int32 [B,7]), views of buffers the next call
  overwrites.  A pixel the matcher rejected reaches the check as NaN and leaves it as code 4; whether it was out of view or not
  unique is in ``matcher``'s own code_l.  After capture() a call is a copy into the static inputs and one graph replay."""

  def __init__(self, height, width, batch=1, maxdisp=192, p1=10, p2=120, paths=8, uniqueness=5, channels=3, tol_abs=1.0,
               tol_rel=0.0, max_diff=1.0, max_size=200, median_radius=0, device="cuda"):
    self.matcher = SemiGlobalMatcher(height, width, batch, maxdisp, p1, p2, paths, uniqueness, channels, device)
    m = self.matcher
    self.median_radius = int_in("ProxyLabeler", "median_radius", median_radius, 0, smooth.MAX_RADIUS)
    # the plain median of either view in front of the check, each gated by the matcher's own code map (0: off, no launch)
    self.medians = tuple(smooth.DisparitySmoother(m.H, m.W, m.B, radius=self.median_radius, device=m.device)
                         for _ in range(2)) if self.median_radius else None
    self.lrc = LeftRightConsistency(m.H, m.W, m.B, tol_abs, tol_rel, device=m.device)
    self.filter = disp_filter.DisparityFilter(m.H, m.W, m.B, max_diff=max_diff, max_size=max_size, device=m.device)
    self._pair = torch.zeros(2 * m.B, m.C, m.H, m.W, dtype=torch.float32, device=m.device)      # static inputs [left; right]
    self._left, self._right = self._pair[:m.B], self._pair[m.B:]
    self._labels = torch.zeros(m.B, 1, m.H, m.W, dtype=torch.float32, device=m.device)
    self._zero = torch.zeros((), dtype=torch.float32, device=m.device)
    self._kept = torch.zeros(m.B, 1, m.H, m.W, dtype=torch.bool, device=m.device)
    self._graph = None
    self._graph_result = None
    self._capture_origin = None

  @torch.no_grad()
  def chain(self, left, right):
    """The chain without the label map, enqueued on the current stream whether or not this object holds a graph: matcher,
    left-right check, speckle pass -> (disp_l, code, counts), views of the matcher's and the filter's buffers.  For a consumer that
    reads the two where they lie (hip_ops.ProxyTermFn: a label iff code == 0 and disp_l > 0) and for a caller that is itself
    being captured: the launches become nodes of ITS graph, on its stream, without a fork.  labels_buffer() is not written."""
    who = "ProxyLabeler.chain"
    self.matcher._check_image(who, "left", left)
    self.matcher._check_image(who, "right", right)
    res, filt = self._chain(left, right)
    return res.disp_l, filt.code, filt.counts

  def _chain(self, left, right):
    res = self.matcher(left, right, fill=float("nan"))
    if self.medians is not None:                                         # a rejected pixel keeps its NaN: code 4 to the check
      res = res._replace(disp_l=self.medians[0](res.disp_l, code_in=res.code_l).disp,
                         disp_r=self.medians[1](res.disp_r, code_in=res.code_r).disp)
    chk = self.lrc.check(res.disp_l, res.disp_r, mirrored=False)
    return res, self.filter.speckles(res.disp_l, chk.code_l)

  def _eager(self, left, right):
    res, filt = self._chain(left, right)
    torch.eq(filt.code, 0, out=self._kept)
    torch.where(self._kept, res.disp_l, self._zero, out=self._labels)
    return self._labels, filt.code, filt.counts

  @torch.no_grad()
  def __call__(self, left, right):
    who = "ProxyLabeler"
    self.matcher._check_image(who, "left", left)
    self.matcher._check_image(who, "right", right)
    if self._graph is not None:
      copy_unless_same(self._left, left)
      copy_unless_same(self._right, right)
      self._graph.replay()
      return self._graph_result
    return self._eager(left, right)

  @torch.no_grad()
  def capture(self, left=None, right=None, labels=None, warmup=1):
    """Records the chain once into a hipGraph (one stream, no forks).  left, right: a pair to warm up on (zeros otherwise).
    labels: the buffer the chain writes its labels into from now on, e.g. a captured trainer's graph_inputs()[2], so that the
    step reads them where they were written."""
    refuse_nested("ProxyLabeler.capture")
    if labels is not None:
      check_f32("ProxyLabeler.capture", "labels", labels, ((4,), "[B,1,H,W]"), device=self._labels.device)
      if tuple(labels.shape) != tuple(self._labels.shape):
        raise RuntimeError("ProxyLabeler.capture: labels must be %s (got %s)" % (tuple(self._labels.shape), tuple(labels.shape)))
      self._labels = labels
    if left is not None:
      self._left.copy_(left)
      self._right.copy_(right)
    self._graph = None
    run = lambda: self._eager(self._left, self._right)
    self._graph, self._graph_result = warm_up_and_capture(run, max(1, warmup), run, owner=self)
    return self

  def captured(self):
    return self._graph is not None

  def inputs(self):
    """The static inputs (left, right) of the captured graph: a caller that fills them itself saves the copy."""
    return self._left, self._right

  def labels_buffer(self):
    return self._labels


def proxy_supervised_step(trainer, labeler, left, right):
  """One supervised step of a training.SupervisedTrainer on the labeler's proxy labels: trainer.step(left, right, labels).  When
  both are captured the labeler's graph is (re)recorded once to write into the trainer's own label input, so that the step's
  replay starts without a copy of the labels."""
  static = trainer.graph_inputs()
  if static is not None and labeler.captured() and tuple(static[2].shape) == tuple(labeler.labels_buffer().shape):
    if labeler.labels_buffer().data_ptr() != static[2].data_ptr():
      labeler.capture(labels=static[2])
    labeler(left, right)
    return trainer.step(left, right, static[2])
  return trainer.step(left, right, labeler(left, right)[0])
