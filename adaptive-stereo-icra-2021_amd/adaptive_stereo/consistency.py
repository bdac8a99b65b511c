"""Both-view inference with the left-right consistency check and the background fill (csrc/lr_consistency.hip).

A single view cannot see its own occlusions: behind a foreground edge, and in the strip the other camera does not cover, the
left disparity is a confident guess.  The remedy is the classical one: predict the right view's disparity as well, keep a left
pixel only if the right pixel it maps to maps back, fill the rest from the background.

  out = predict_disparity_leftright(feature_net, stereo_net, left, right)     # the reference's dictionary, for a whole batch
  lrc = LeftRightConsistency(H, W, batch=B)
  chk = lrc.check(out["pred_disp_l/0"], out["pred_disp_r/0"])                 # LRCheck: codes, valid maps, |d - r|, counts
  filled = lrc.fill(out["pred_disp_l/0"], chk.code_l)
  cloud = proj.voxel_cloud(out["pred_disp_l/0"], left, confidence=chk.valid_l, conf_min=1.0)   # pointcloud.DepthProjector

  both = BothViewInference(feature_net, stereo_net, H, W, batch=B).capture()  # all of the above as one hipGraph replay
  disp_l, disp_r, chk, filled_l = both(left, right)

The reference holds only the first line (adapt.py:40-62); the loss that was to consume it is dead code there and stays out
(adapt.py's --leftright_consistency still raises).  The arithmetic of the check is fixed op by op in
include/adaptive_stereo_hip.h.  There is no CPU path.
"""
import collections

import numpy as np
import torch

from . import _native as nat
from . import hip_ops
from .capture import copy_unless_same, refuse_nested, warm_up_and_capture
from .collect import MapOperator, check_f32, check_u8

CODE_NAMES = ("consistent", "occluded", "mismatch", "out_of_view", "bad_input")

LRCheck = collections.namedtuple("LRCheck", "code_l code_r valid_l valid_r diff_l diff_r counts")


def _check_pair(who, left, right):
  check_f32(who, "left", left, ((4,), "[B,C,H,W]"))
  check_f32(who, "right", right, ((4,), "[B,C,H,W]"), device=left.device)
  if left.shape != right.shape or min(left.shape) < 1:
    raise RuntimeError("%s: left %s and right %s must have one non-empty shape" % (who, tuple(left.shape), tuple(right.shape)))


def mirror_pair(left, right, out=None):
  """(left_batch, right_batch) = ([left; right mirrored in x], [right; left mirrored in x]), the two halves of ONE buffer
  [4B,C,H,W] (`out`, allocated when None), so that FeatureExtractorNetwork.forward_pair needs no concatenation.  One launch."""
  _check_pair("mirror_pair", left, right)
  B, C, H, W = left.shape
  if out is None:
    out = torch.empty(4 * B, C, H, W, dtype=torch.float32, device=left.device)
  else:
    check_f32("mirror_pair", "out", out, ((4,), "[4B,C,H,W]"), device=left.device, numel=4 * left.numel())
  with torch.cuda.device(left.device):
    nat.call("as_mirror_pair", nat.ptr(left.detach()), nat.ptr(right.detach()), B, C, H, W, nat.ptr(out),
             nat.c_vp(out.data_ptr() + 8 * left.numel()), nat.stream())
  return out[:2 * B], out[2 * B:]


def flip_w(src, out=None):
  """A contiguous fp32 tensor [..., H, W] mirrored in x, out of place.  One launch."""
  check_f32("flip_w", "src", src, ((2, 3, 4, 5), "[...,H,W]"))
  if src.numel() < 1:
    raise RuntimeError("flip_w: empty input %s" % (tuple(src.shape),))
  if out is None:
    out = torch.empty_like(src)
  else:
    check_f32("flip_w", "out", out, device=src.device, numel=src.numel())
  H, W = src.shape[-2:]
  with torch.cuda.device(src.device):
    nat.call("as_flip_w", nat.ptr(src.detach()), src.numel() // (H * W), H, W, nat.ptr(out), nat.stream())
  return out


def predict_disparity_leftright(feature_net, stereo_net, left, right, output_cost_volume=False):
  """The reference's predict_disparity_leftright (adapt.py:40-62) for a batch of B pairs: one as_mirror_pair, one
  feature_net.forward_pair, one stereo_net(..., "x", ...).  Every ``_x`` key of the network's outputs appears once as ``_l`` (the
  first B entries) and once as ``_r`` (the last B, mirrored back by as_flip_w).  Inference only: under no_grad, and a network in
  training mode is refused, because its batch statistics would mix the two views."""
  if feature_net.training or stereo_net.training:
    raise RuntimeError("predict_disparity_leftright: inference only; call .eval() on both networks (in training mode the "
                       "BatchNorm statistics of a batch would mix the two views)")
  with torch.no_grad():
    left_batch, right_batch = mirror_pair(left, right)
    B = left.shape[0]
    fl, fr = feature_net.forward_pair(left_batch, right_batch)
    outputs = stereo_net(left_batch, fl, fr, "x", output_cost_volume=output_cost_volume)
    outputs_lr = {}
    for key, value in outputs.items():
      outputs_lr[key.replace("_x", "_l")] = value[:B]
      outputs_lr[key.replace("_x", "_r")] = flip_w(value[B:].contiguous())
  return outputs_lr


class LeftRightConsistency(MapOperator):
  """The check and the fill for maps [batch,1,height,width].  All output buffers are allocated once; every call overwrites them,
  enqueues only and is graph-capturable.  tol = max(tol_abs, tol_rel * d) in disparity units."""

  def __init__(self, height, width, batch=1, tol_abs=1.0, tol_rel=0.0, device="cuda"):
    super().__init__(height, width, batch, device)
    self.tol_abs, self.tol_rel = float(tol_abs), float(tol_rel)
    if not (np.isfinite(self.tol_abs) and np.isfinite(self.tol_rel) and self.tol_abs >= 0 and self.tol_rel >= 0):
      raise ValueError("LeftRightConsistency: tol_abs %r and tol_rel %r must be finite and not negative" % (tol_abs, tol_rel))
    shape = (2, self.B, 1, self.H, self.W)                 # left view, right view
    self._code = self._zeros(shape, torch.uint8)
    self._valid = self._zeros(shape, torch.float32)
    self._diff = self._zeros(shape, torch.float32)
    self._counts = self._zeros((self.B, 2, len(CODE_NAMES)), torch.int32)
    self._filled = self._zeros(shape[1:], torch.float32)
    self._result = LRCheck(self._code[0], self._code[1], self._valid[0], self._valid[1], self._diff[0], self._diff[1], self._counts)

  def check(self, disp_l, disp_r, mirrored=False):
    """LRCheck of views into this object's buffers: code_l, code_r (uint8: 0 consistent, 1 occluded, 2 mismatch, 3 out of view,
    4 bad input), valid_l, valid_r (fp32 1.0 / 0.0: the `confidence` of DepthProjector.organized / voxel_cloud with
    conf_min=1.0), diff_l, diff_r (|d - r|, NaN for codes 3 and 4), counts (int32 [B,2,5]).  mirrored=True: disp_r is the
    second half of the network's output for the mirrored pair as it is, not flipped back; the results are the same bits."""
    self._check_map("LeftRightConsistency.check", "disp_l", disp_l)
    self._check_map("LeftRightConsistency.check", "disp_r", disp_r)
    r = self._result
    with torch.cuda.device(self.device):
      nat.call("as_lr_check", nat.ptr(disp_l.detach()), nat.ptr(disp_r.detach()), int(bool(mirrored)), self.B, self.H, self.W,
               self.tol_abs, self.tol_rel, nat.ptr(r.code_l), nat.ptr(r.code_r), nat.ptr(r.valid_l), nat.ptr(r.valid_r),
               nat.ptr(r.diff_l), nat.ptr(r.diff_r), nat.ptr(r.counts), nat.stream())
    return r

  def fill(self, disp, code, out=None):
    """disp where code is 0; elsewhere the smaller of the nearest code-0 values to the left and to the right in the row (the
    background), the only one where one side has none, 0.0 in a row without any.  out: this object's buffer when None."""
    who = "LeftRightConsistency.fill"
    self._check_map(who, "disp", disp)
    check_u8(who, "code", code, disp.shape, disp.device)
    if out is None:
      out = self._filled
    else:
      self._check_map(who, "out", out)
    if out.data_ptr() == disp.data_ptr():
      raise RuntimeError("%s: out may not alias disp" % who)
    with torch.cuda.device(self.device):
      nat.call("as_lr_fill", nat.ptr(disp.detach()), nat.ptr(code), self.B, self.H, self.W, nat.ptr(out), nat.stream())
    return out

  def fractions(self):
    """Synchronises.  numpy fp64 [B,2,5]: the share of each code per image and view in the last check()."""
    return self._fractions(self._counts)


class BothViewInference(object):
  """Mirror, one forward pass over both views, the check on the network's own (still mirrored) right-view output, the flip back
  and the fill of the left view, on buffers allocated once.  ``__call__(left, right)`` -> (disp_l, disp_r, LRCheck, filled_l),
  views of this object's buffers that the next call overwrites.  After capture() a call is a copy into the static inputs and one
  graph replay."""

  def __init__(self, feature_net, stereo_net, height, width, batch=1, tol_abs=1.0, tol_rel=0.0, channels=3):
    self.feature_net, self.stereo_net = feature_net, stereo_net
    if stereo_net.input_scale != 0:
      raise ValueError("BothViewInference: the check runs on the full-resolution maps [B,1,height,width]; a StereoNet with "
                       "input_scale %r predicts at another size (only input_scale 0 is supported)" % (stereo_net.input_scale,))
    dev = next(stereo_net.parameters()).device
    self.lrc = LeftRightConsistency(height, width, batch, tol_abs, tol_rel, device=dev)
    B, H, W = self.lrc.B, self.lrc.H, self.lrc.W
    self._pair = torch.zeros(2 * B, int(channels), H, W, dtype=torch.float32, device=dev)        # static inputs [left; right]
    self._left, self._right = self._pair[:B], self._pair[B:]
    self._batches = torch.zeros(4 * B, int(channels), H, W, dtype=torch.float32, device=dev)     # [left_batch; right_batch]
    self._disp_r = torch.zeros(B, 1, H, W, dtype=torch.float32, device=dev)
    self.plan = hip_ops.StepPlan()          # the eval-mode forward's packing in one launch, as OnlineAdapter.infer_plan
    self._graph = None
    self._graph_result = None
    self._capture_origin = None
    self.scale = "pred_disp_x/0"

  @torch.no_grad()
  def __call__(self, left, right):
    _check_pair("BothViewInference", left, right)
    if tuple(left.shape) != tuple(self._left.shape) or left.device != self._pair.device:
      raise RuntimeError("BothViewInference: built for pairs %s on %s (got %s on %s)"
                         % (tuple(self._left.shape), self._pair.device, tuple(left.shape), left.device))
    if self._graph is not None:
      copy_unless_same(self._left, left)
      copy_unless_same(self._right, right)
      self._graph.replay()
      return self._graph_result
    return self._eager(left, right)

  def _forward_and_check(self, left, right):
    """-> (disp_l, the right view's disparity still mirrored, LRCheck); disp_filter.FilteredBothViewInference shares it"""
    if self.feature_net.training or self.stereo_net.training:
      raise RuntimeError("BothViewInference: inference only; call .eval() on both networks")
    B = self.lrc.B
    left_batch, right_batch = mirror_pair(left, right, out=self._batches)
    self.plan.begin()
    try:
      fl, fr = self.feature_net.forward_pair(left_batch, right_batch)
      disp = self.stereo_net(left_batch, fl, fr, "x")[self.scale]
    finally:
      self.plan.end()
    disp_l, mirrored_r = disp[:B], disp[B:]
    return disp_l, mirrored_r, self.lrc.check(disp_l, mirrored_r, mirrored=True)

  def _eager(self, left, right):
    disp_l, mirrored_r, chk = self._forward_and_check(left, right)
    flip_w(mirrored_r, out=self._disp_r)
    return disp_l, self._disp_r, chk, self.lrc.fill(disp_l, chk.code_l)

  @torch.no_grad()
  def capture(self, left=None, right=None, warmup=2):
    """Records the sequence once into a hipGraph (one stream, no forks); left, right: a pair to warm up on (zeros otherwise)."""
    refuse_nested("BothViewInference.capture")
    if left is not None:
      self._left.copy_(left)
      self._right.copy_(right)
    run = lambda: self._eager(self._left, self._right)
    # (warm-up: the first call records the plan, the second runs it)
    self._graph, self._graph_result = warm_up_and_capture(run, max(2, warmup), run, owner=self)
    return self

  def inputs(self):
    """The static inputs (left, right) of the captured graph: a caller that fills them itself saves the copy."""
    return self._left, self._right

  @torch.no_grad()
  def run_static(self):
    """The chain, eagerly, on the static inputs as they stand: for a stage in front that fills inputs() itself and records the
    whole sequence in a capture of its own (rectify.RectifiedInference)."""
    return self._eager(self._left, self._right)
