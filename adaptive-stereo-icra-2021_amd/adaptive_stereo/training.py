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
from . import hip_ops
from .adaptation import FlatArena, FusedClipAdam
from .capture import copy_unless_same, refuse_nested, static_pair, warm_up_and_capture
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
    # (the weight-gradient reductions of the step run as one launch when the region closes; bn_sync=None changes nothing: this
    # trainer has no cross-replica BatchNorm)
    with hip_ops.step_region(self.plan, bn_sync=None):
      # each image with its own BatchNorm statistics, as two passes of the feature extractor have (train.py:20)
      fl, fr = self.feature_net.forward_pair(left, right)
      out = self.stereo_net(left, fl, fr, "l")
      losses = self._losses(gt, out)
      losses["total_loss"].backward()
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
    from then on (the capture rules: capture.py; forward_pair never forks, so there is no capture origin to record).  Inputs are
    copied into static buffers before a replay unless they already are those buffers (graph_inputs()).  The warm-up steps are
    undone: parameters, moments, step count and BatchNorm buffers are what they were before the call."""
    refuse_nested("SupervisedTrainer.capture")
    self._graph = None
    self._static = static_pair(left, right) + (gt.clone(),)
    count = self.optimizer.step_count
    step = lambda: self._step_eager(*self._static)
    # (warm-up: the first step a plan sees records it, the next one runs it)
    self._graph, self._static_result = warm_up_and_capture(step, max(2, warmup), step, state=self._state_tensors)
    self.optimizer.step_count = count          # capture only records, and the warm-up is undone
    return self

  def _replay(self, left, right, gt):
    for dst, src in zip(self._static, (left, right, gt)):
      copy_unless_same(dst, src)
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
