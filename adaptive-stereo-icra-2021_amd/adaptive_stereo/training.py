"""One supervised training step, as the reference's train.py performs it (train.py:204-223), on MI355X.

Reference sequence:
  feature_net(left), feature_net(right) -> stereo_net(left, fl, fr, "l")
  -> khamis_robust_loss_multiscale(scales=[s, s + k]) -> zero_grad, total_loss.backward()
  -> [clip_grad_norm_(stereo_net.parameters(), 1.0)] -> Adam.step();  StepLR(scheduler_step_size, 0.5) per epoch

Same arrangement as the adaptation step (adaptation.py): parameters, gradients and both Adam moments in flat arenas
(stereo_net first, then feature_net: train.py:165), the backward kernels add into the gradient arena, clip + Adam are
FusedClipAdam, the whole step is captured into one hipGraph.  What is particular to supervised training:
  * the two-scale loss is one autograd node (hip_ops.SupervisedLossFn): one pass over the ground truth forward; backward, the
    coarse term's gradient reaches the soft-argmax output through the up-sampling adjoint without its full-resolution
    derivative map ever being stored;
  * the learning rate lives on the device (as_adam_step_lr), so the captured step follows StepLR through set_lr();
  * capture() leaves the training state exactly as it found it: its warm-up steps are undone, so a run that captures after
    its first batch computes what a run of eager steps computes, bit for bit.
The step issues no host sync.
"""
import torch

from . import hip_ops
from .adaptation import FlatArena, FusedClipAdam
from .utils.loss_functions import khamis_robust_loss_two_scale


class SupervisedTrainer(object):
  """feature_net + stereo_net + optimiser bound together for the supervised step."""

  def __init__(self, feature_net, stereo_net, lr=1e-5, clip_grad_norm=False):
    self.feature_net, self.stereo_net = feature_net, stereo_net
    self.scale = stereo_net.input_scale
    self.coarse_scale = stereo_net.input_scale + stereo_net.k
    self.clip = bool(clip_grad_norm)
    self.arena = FlatArena([stereo_net, feature_net])      # train.py:165 order
    self.optimizer = FusedClipAdam(self.arena, lr, lr_on_device=True)
    self.plan = hip_ops.StepPlan()
    self._graph = None
    self._static = None
    self._static_result = None

  # -- one step: train.py:204-223 -----------------------------------------------------------------------
  def step(self, left, right, gt):
    """-> {"total_loss", "khamis_robust_loss/{s}", "khamis_robust_loss/{s+k}"} (device scalars) and "outputs"."""
    if self._graph is not None and tuple(left.shape) == tuple(self._static[0].shape):
      return self._replay(left, right, gt)
    return self._step_eager(left, right, gt)        # (a batch of another size: with drop_last=False the last of an epoch)

  def _step_eager(self, left, right, gt):
    self.feature_net.train(); self.stereo_net.train()
    self.arena.rebind_grads()
    self.arena.zero_grads()
    self.plan.begin()
    hip_ops.rmw_order_reset(True)        # (the weight-gradient reductions of the step run as one launch when it closes)
    try:
      # each image with its own BatchNorm statistics, as two passes of the feature extractor have (train.py:20)
      fl, fr = self.feature_net.forward_pair(left, right)
      out = self.stereo_net(left, fl, fr, "l")
      losses = self._losses(gt, out)
      losses["total_loss"].backward()
    finally:
      hip_ops.rmw_order_reset(False)
      self.plan.end()
    self.optimizer.step(clip=self.clip)
    result = {name: value.detach() for name, value in losses.items()}
    result["outputs"] = out
    return result

  def _losses(self, gt, out):
    return khamis_robust_loss_two_scale({"gt_disp_l/{}".format(self.scale): gt}, out, self.scale, self.coarse_scale, self.scale)

  def set_lr(self, lr):
    """The learning rate from the next step on (a device scalar: a captured step reads it on its next replay)."""
    self.optimizer.set_lr(lr)

  # -- hipGraph capture of the whole step ---------------------------------------------------------------------
  def _state_tensors(self):
    """name -> tensor of everything a step changes.  Looked up anew at each use: a StepPlan re-homes the BatchNorm batch
    counters when it is built (same state_dict keys, other tensors)."""
    opt = self.optimizer
    state = {"params": self.arena.params, "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq, "step": opt.step_dev,
             "sumsq": opt.sumsq, "coef": opt.coef}
    for prefix, net in (("stereo.", self.stereo_net), ("feature.", self.feature_net)):
      for name, b in net.named_buffers():
        state[prefix + name] = b
    return state

  def capture(self, left, right, gt, warmup=2):
    """Captures one step (forward, loss, backward, [clip,] Adam) for batches of this shape into a hipGraph; step() replays it
    from then on.  Discipline of OnlineAdapter.capture: warm-up on a side stream, capture on that stream,
    capture_error_mode="thread_local", no capture inside a capture; inputs are copied into static buffers before a replay
    unless they already are those buffers (graph_inputs()).  The warm-up steps are undone: parameters, moments, step count and
    BatchNorm buffers are what they were before the call."""
    if torch.cuda.is_current_stream_capturing():
      raise RuntimeError("SupervisedTrainer.capture: the current stream is already being captured; a capture inside a "
                         "capture crashes hipStreamEndCapture on ROCm 7.2 — capture from an ordinary stream")
    pair = torch.cat([left, right])      # one buffer, the two images its halves: the pair pass needs no concatenation copy
    self._graph = None
    self._static = (pair[:left.shape[0]], pair[left.shape[0]:], gt.clone())
    saved = {name: t.clone() for name, t in self._state_tensors().items()}
    count = self.optimizer.step_count
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      for _ in range(max(2, warmup)):          # the first step a plan sees records it, the next one runs it
        self._step_eager(*self._static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):   # the warm-up's stream: its pooled
      self._static_result = self._step_eager(*self._static)                          # buffers are reused
    with torch.no_grad():
      for name, t in self._state_tensors().items():
        t.copy_(saved[name])
    self.optimizer.step_count = count          # capture only records, and the warm-up is undone
    self._graph = graph
    return self

  def _replay(self, left, right, gt):
    for src, dst in zip((left, right, gt), self._static):
      if src.data_ptr() != dst.data_ptr():
        dst.copy_(src)
    self._graph.replay()
    self.optimizer.step_count += 1          # host mirror of the device-side counter
    return self._static_result

  def graph_count(self):
    """hipGraphs a captured step replays (0: eager stepping)."""
    return 0 if self._graph is None else 1

  def graph_inputs(self):
    """The captured step's own input buffers (left, right, gt): a producer that fills them and passes them to step() saves
    the copies a replay otherwise starts with."""
    return self._static
