"""Adaptation control plane: states, online validation set (OVS), FCS-EMA out-of-distribution gate,
experience replay.  SURVEY.md §8f-2.

Reference: adapt.py — ``State`` (:34-37), ``StateMachine`` (:89-172) and the per-batch logic of
``adapt()`` (:290-396).  This is host-side control; every tensor op it triggers is one of the HIP
operators.  Differences in form: validation takes the loss function as a callable, the OOD decision is
the only place that reads a device scalar back (and only in the VS / VS+ER modes, which need the
decision on the host to route the pair into the reservoir), and the per-step work is delegated to
``OnlineAdapter``.

``AdaptationLoop(..., captured=True)`` takes the three per-step decisions (novel or not, which reservoir slot if any, update
or not) on the device instead (csrc/adapt_gate.hip: as_adapt_gate, as_reservoir_store; the gated clip + Adam of csrc/optim.hip)
and replays an IN_PROGRESS step of every mode as ONE hipGraph without a host read-back; the reservoir is a ``DeviceReservoir``.
Validation and ``StateMachine.transition`` stay on the host, at the loop's sync points.
"""
import random
from enum import Enum

import torch

from . import _native as nat
from .capture import refuse_nested, static_pair, warm_up_and_capture
from .utils.stereo_reservoir import StereoReservoir

MODES = ("NONSTOP", "VS", "ER", "VS+ER", "NONE")
OVS_METRICS = ("photometric", "proxy_epe")


class State(Enum):
  DONE = 0          # adaptation finished: no gradient updates
  IN_PROGRESS = 1   # adapting
  VALIDATION = 2    # scoring the OVS: gradients off


class StateMachine(object):
  def __init__(self, initial_state, ovs_buffer_size=8, verbose=False):
    self.initial_state = initial_state
    self.current_state = initial_state
    self.ovs = StereoReservoir(ovs_buffer_size)
    self.prev_ovs_loss = float("inf")
    self.ovs_did_change = True
    self.ovs_iters_without_improvement = 0
    self.verbose = verbose

  def state(self):
    return self.current_state

  def ovs_buffer_size(self):
    return self.ovs.size()

  def restart(self):
    self.current_state = self.initial_state

  def add_to_ovs(self, left_img, right_img, loss, batch_idx):
    """Offers a (novel) pair to the reservoir; a DONE machine is restarted by any offer (adapt.py:101-115)."""
    did_add = self.ovs.add(left_img.detach(), right_img.detach(), loss.detach() if torch.is_tensor(loss) else loss,
                           batch_idx)
    if did_add:
      self.ovs_did_change = True
    if self.current_state == State.DONE:
      self.restart()
    return did_add

  def validate(self, loss_fn):
    """Re-scores every buffered pair with the current weights.  ``loss_fn(left, right) -> float`` must run
    the networks in eval mode without gradients (adapt.py:121-142)."""
    for i in range(self.ovs.size()):
      _, _, left, right = self.ovs.buf[i]
      self.ovs.update_value(i, float(loss_fn(left, right)))

  def transition(self, val_improve_retries):
    """adapt.py:144-166: stop when the OVS loss did not improve for `val_improve_retries` validations in a
    row while the buffer was unchanged; otherwise (improved, or buffer changed) keep adapting."""
    ovs_loss = float(self.ovs.average_value())
    if ovs_loss >= self.prev_ovs_loss and not self.ovs_did_change:
      self.ovs_iters_without_improvement += 1
      if self.ovs_iters_without_improvement >= val_improve_retries:
        self.current_state = State.DONE
        self.prev_ovs_loss = float("inf")
    else:
      self.ovs_did_change = False
      self.ovs_iters_without_improvement = 0
      self.prev_ovs_loss = ovs_loss
    return self.current_state


class _SlotView(object):
  """``DeviceReservoir.buf``: entry i as StereoReservoir's [value, index, left, right] (views of the device buffers).  The index
  is the one the slot was appended with: a replacement keeps it, as it keeps the reference's index set."""

  def __init__(self, owner):
    self._o = owner

  def __len__(self):
    return self._o.size()

  def __getitem__(self, i):
    o = self._o
    n = len(self)
    if not -n <= i < n:
      raise IndexError("reservoir slot %d of %d" % (i, n))
    i %= n
    return [o.values[i], int(o.indices[i]), o.left[i], o.right[i]]


class DeviceReservoir(object):
  """StereoReservoir with its pairs, values and bookkeeping in device memory, filled by as_adapt_gate / as_reservoir_store
  (see include/adaptive_stereo_hip.h for the exact semantics: those of StereoReservoir.add, with random.randint(1, offers)
  drawn as 1 + min(int(u * offers), offers - 1) from one uniform double per step).

  state   int64 [size, offers, adds, updates]        indices int32 [capacity]      values fp32 [capacity]
  left / right  fp32 [capacity, B, C, H, W], allocated when the first batch shows its shape
  out3    int32 [novel, slot, update] of the last step

  size(), average_value(), update_value() and buf[i] are StereoReservoir's, so StateMachine.validate / transition work on it
  unchanged; each of them except update_value reads the device (a host synchronisation)."""

  def __init__(self, max_size, device="cuda"):
    if max_size < 1:
      raise ValueError("DeviceReservoir: capacity must be at least 1")
    self.max_size = int(max_size)
    dev = torch.device(device)
    self.state = torch.zeros(4, dtype=torch.int64, device=dev)
    self.indices = torch.zeros(self.max_size, dtype=torch.int32, device=dev)
    self.values = torch.zeros(self.max_size, dtype=torch.float32, device=dev)
    self.out3 = torch.zeros(3, dtype=torch.int32, device=dev)
    self.left = self.right = None
    self._offered = False          # no launch of the gate yet: the size is 0 without asking the device
    self.buf = _SlotView(self)

  def allocate(self, like):
    if self.left is None:
      self.left = torch.zeros((self.max_size,) + tuple(like.shape), dtype=torch.float32, device=self.state.device)
      self.right = torch.zeros_like(self.left)
    elif tuple(self.left.shape[1:]) != tuple(like.shape):
      raise ValueError("DeviceReservoir: batches of %s, allocated for %s" % (tuple(like.shape), tuple(self.left.shape[1:])))

  # -- the two launches of a step (enqueue only) ----------------------------------------------------
  def gate(self, fcs_smoothed, loss, batch_idx, u, threshold, gate_enabled, adapting):
    self._offered = True
    nat.call("as_adapt_gate", nat.ptr(fcs_smoothed), nat.ptr(loss), nat.ptr(batch_idx), nat.ptr(u), float(threshold),
             self.max_size, int(bool(gate_enabled)), int(bool(adapting)), nat.ptr(self.state), nat.ptr(self.indices),
             nat.ptr(self.values), nat.ptr(self.out3), nat.stream())

  def store(self, left, right):
    nat.call("as_reservoir_store", nat.ptr(left), nat.ptr(right), left.numel(), nat.ptr(self.out3[1:2]), self.max_size,
             nat.ptr(self.left), nat.ptr(self.right), nat.stream())

  # -- StereoReservoir's interface ------------------------------------------------------------------
  def counters(self):
    """(size, offers, adds, updates) as python ints."""
    return tuple(int(v) for v in self.state.cpu().tolist())

  def size(self):
    if not self._offered:
      return 0
    return int(self.state[0])

  @property
  def i(self):
    return int(self.state[1])

  def update_value(self, buf_index, new_value):
    self.values[buf_index:buf_index + 1].fill_(float(new_value))

  def average_value(self):
    vals = self.values[:self.size()].cpu().tolist()
    return sum(vals) / len(vals)


class AdaptationLoop(object):
  """The body of the reference's ``for inputs in adapt_loader`` (adapt.py:290-396) around an OnlineAdapter.

  mode                NONSTOP | VS | ER | VS+ER | NONE
  ovs_validate_hz     validate the OVS every this many steps (while IN_PROGRESS and non-empty)
  val_improve_retries see StateMachine.transition
  ood_threshold       a pair is novel when the smoothed FCS is below it
  er_loss_weight      weight of the Khamis loss on the replayed training pair (ER modes)
  captured            the gated step (below); off, the loop is the host-side one and its results are unchanged
  ovs_metric          "photometric": the reservoir is validated by OnlineAdapter.validation_loss (the reference's);
                      "proxy_epe": by OnlineAdapter.validation_proxy_epe, the mean distance to the semi-global matcher's labels
                      (needs an adapter with a proxy_labeler; a stored pair without a single label scores by its photometric
                      loss: see there).  Either runs every ovs_validate_hz steps, where the loop synchronises anyway.

  captured=True.  An IN_PROGRESS step is forward_loss, as_adapt_gate, as_reservoir_store, backward_update with the gated
  optimizer: the same call sequence as the host loop, always including backward, with the update withheld on the device when the
  pair went into the reservoir.  The first such step runs eagerly (it creates the FCS EMA and records the step plan), the second
  is captured, every later one replays the graph: inputs are copied into static buffers, ``batch_idx`` and the step's uniform
  number ``u`` reach the device by fill_ (kernel arguments), and nothing is read back.  result["updated"] and
  result["added_to_ovs"] are 0-d device tensors.  ``gradient_updates`` and ``optimizer.step_count`` are refreshed from the device
  at the sync points: every ``ovs_validate_hz`` steps (before validation), in DONE-state steps, and by sync() — call it before
  ``optimizer.state_dict()`` / save_models.  DONE-state steps stay eager: they run as_adapt_gate with adapting = 0 and read
  ``novel`` back to restart the machine, as StateMachine.add_to_ovs does.
  Random numbers: the VS modes draw one random.random() per gated step; the host loop draws random.randint only on an offer to a
  full buffer.  Both sample the reference's distribution; from one seed the two loops follow different sequences.
  In the ER modes the replay triple must be given on every step or on none (one graph).  Single GPU only."""

  def __init__(self, adapter, mode="NONSTOP", ovs_buffer_size=10, ovs_validate_hz=100, val_improve_retries=1,
               ood_threshold=15.0, er_loss_weight=0.05, captured=False, ovs_metric="photometric"):
    if mode not in MODES:
      raise ValueError("adapt_mode must be one of %s" % (MODES,))
    if ovs_metric not in OVS_METRICS:
      raise ValueError("ovs_metric must be one of %s" % (OVS_METRICS,))
    if ovs_metric == "proxy_epe" and getattr(adapter, "proxy_labeler", None) is None:
      raise ValueError("AdaptationLoop(ovs_metric=\"proxy_epe\") needs an adapter with a proxy_labeler")
    self.ovs_metric = ovs_metric
    if captured and getattr(adapter, "dp", False):
      raise NotImplementedError("AdaptationLoop(captured=True) is single-GPU: a data-parallel adapter decides the gate on "
                                "all-reduced scalars, which the captured step does not do; use captured=False")
    self.adapter = adapter
    self.mode = mode
    self.ovs_validate_hz = ovs_validate_hz
    self.val_improve_retries = val_improve_retries
    self.ood_threshold = ood_threshold
    self.er_loss_weight = er_loss_weight
    initial = State.DONE if mode == "NONE" else State.IN_PROGRESS
    self.state_machine = StateMachine(initial, ovs_buffer_size=ovs_buffer_size)
    self.step = 0
    self.gradient_updates = 0
    self.captured = bool(captured)
    if self.captured:
      dev = adapter.arena.params.device
      self.state_machine.ovs = DeviceReservoir(ovs_buffer_size, dev)
      self._batch_idx = torch.zeros(1, dtype=torch.int32, device=dev)
      self._u = torch.zeros(1, dtype=torch.float64, device=dev)
      self._static = None            # (left, right, replay triple or None): the captured step's own input buffers
      self._graph = None
      self._graph_result = None
      self._use_replay = None
      self._adds_seen = 0

  def _validation_loss(self, left, right):
    if self.ovs_metric == "proxy_epe":
      return self.adapter.validation_proxy_epe(left, right)
    return self.adapter.validation_loss(left, right)

  def process(self, left, right, batch_idx, replay=None):
    """One batch.  ``replay`` = (left, right, gt_disp) of a training-domain pair for the ER modes."""
    if self.captured:
      return self._process_captured(left, right, batch_idx, replay)
    sm = self.state_machine
    if (self.step % self.ovs_validate_hz == 0) and sm.ovs_buffer_size() > 0 and sm.state() == State.IN_PROGRESS:
      sm.validate(self._validation_loss)
      if self.mode not in ("NONSTOP", "ER", "NONE"):
        sm.transition(self.val_improve_retries)

    adapting = sm.state() == State.IN_PROGRESS
    use_replay = self.mode in ("ER", "VS+ER") and replay is not None
    gate = self.mode not in ("NONSTOP", "ER", "NONE")
    # Forward (+ loss) first; whether the backward/optimizer part runs is decided after the OOD gate.
    result = self.adapter.forward_loss(left, right, train=adapting, replay=replay if use_replay else None,
                                       er_loss_weight=self.er_loss_weight)
    did_add = False
    if gate:
      novel = float(result["fcs_smoothed"]) < self.ood_threshold          # the one host read-back (VS modes)
      if novel:
        did_add = bool(sm.add_to_ovs(left, right, result["loss"], batch_idx))
    updated = False
    if sm.state() == State.IN_PROGRESS and adapting and not did_add:
      self.adapter.backward_update(result)
      self.gradient_updates += 1
      updated = True
    self.step += 1
    result.update(state=sm.state(), added_to_ovs=did_add, updated=updated)
    return result

  # -- captured=True ---------------------------------------------------------------------------------------------------
  def sync(self):
    """Refreshes the host mirrors of what gated steps count on the device (a host synchronisation): gradient_updates,
    optimizer.step_count, and whether the reservoir changed since the last transition."""
    if not self.captured:
      return
    _, _, adds, updates = self.state_machine.ovs.counters()
    if adds != self._adds_seen:
      self._adds_seen = adds
      self.state_machine.ovs_did_change = True
    self.gradient_updates = updates
    self.adapter.optimizer.refresh_step_count()

  def graph_count(self):
    return 0 if not self.captured or self._graph is None else 1

  def _bind_inputs(self, left, right, replay):
    if self._static is None:
      sl, sr = static_pair(left, right)
      srep = None if replay is None else static_pair(replay[0], replay[1]) + (replay[2].clone(),)
      self._static = (sl, sr, srep)
      self.state_machine.ovs.allocate(sl)
      return
    sl, sr, srep = self._static
    sl.copy_(left); sr.copy_(right)
    if srep is not None:
      for dst, src in zip(srep, replay):
        dst.copy_(src)

  def _gated_body(self, threshold, gate_enabled, adapting):
    """forward_loss, gate, store, backward_update on the static inputs: what the graph holds."""
    sl, sr, srep = self._static
    ovs = self.state_machine.ovs
    result = self.adapter.forward_loss(sl, sr, train=True, replay=srep, er_loss_weight=self.er_loss_weight)
    ovs.gate(result["fcs_smoothed"], result["loss"], self._batch_idx, self._u, threshold, gate_enabled, adapting)
    ovs.store(sl, sr)
    self.adapter.backward_update(result, gate=ovs.out3[2:3])
    result["updated"] = ovs.out3[2]
    result["added_to_ovs"] = ovs.out3[1] >= 0
    result["novel"] = ovs.out3[0]
    return result

  def _capture(self, gate_enabled):
    """Warm-up on the capture stream with the gate shut (nothing is novel, nothing adapts: the reservoir, the parameters, both
    moments and the step count stay as they are), then the capture.  What a forward pass in train mode changes on its own — the
    BatchNorm running statistics and counters, the FCS EMA — is put back afterwards, so the loop's state is the one it had.
    (The loop captures only once the adapter's step plan is built, so the buffers saved are the buffers the graph updates.)"""
    a = self.adapter
    refuse_nested("AdaptationLoop capture")

    def state():
      named = {prefix + name: b for prefix, net in (("stereo.", a.stereo_net), ("feature.", a.feature_net))
               for name, b in net.named_buffers()}
      named["fcs_ema"] = a.fcs_smoothed
      return named

    self._graph, self._graph_result = warm_up_and_capture(
      lambda: self._gated_body(float("-inf"), False, False), 2,
      lambda: self._gated_body(self.ood_threshold, gate_enabled, True), owner=a, state=state)

  def _process_captured(self, left, right, batch_idx, replay):
    sm = self.state_machine
    if self.step % self.ovs_validate_hz == 0 and sm.state() == State.IN_PROGRESS:
      self.sync()
      if sm.ovs_buffer_size() > 0:
        sm.validate(self._validation_loss)
        if self.mode not in ("NONSTOP", "ER", "NONE"):
          sm.transition(self.val_improve_retries)

    adapting = sm.state() == State.IN_PROGRESS
    use_replay = self.mode in ("ER", "VS+ER") and replay is not None
    gate = self.mode not in ("NONSTOP", "ER", "NONE")
    if self._use_replay is None:
      self._use_replay = use_replay
    elif adapting and use_replay != self._use_replay:
      raise ValueError("AdaptationLoop(captured=True): the replay triple must be given on every step or on none")
    self._batch_idx.fill_(int(batch_idx))
    if gate:
      self._u.fill_(random.random())
    if adapting:
      self._bind_inputs(left, right, replay if use_replay else None)
      if self._graph is None and self.adapter.fcs_smoothed is not None and self.adapter.plan.ready:
        self._capture(gate)
      if self._graph is not None:
        self._graph.replay()
        result = dict(self._graph_result)
      else:
        result = self._gated_body(self.ood_threshold, gate, True)
    else:
      # DONE: eval-mode forward without gradients, the gate with adapting = 0, and the one read-back that can restart the machine
      ovs = sm.ovs
      ovs.allocate(left)
      result = self.adapter.forward_loss(left, right, train=False, replay=replay if use_replay else None,
                                         er_loss_weight=self.er_loss_weight)      # (the replay loss is still reported, as by the host loop)
      ovs.gate(result["fcs_smoothed"], result["loss"], self._batch_idx, self._u, self.ood_threshold, gate, False)
      ovs.store(left.contiguous(), right.contiguous())
      result["updated"] = ovs.out3[2].clone()
      result["added_to_ovs"] = ovs.out3[1] >= 0
      result["novel"] = ovs.out3[0].clone()
      if gate and int(ovs.out3[0]) != 0:
        sm.restart()
      self.sync()
    self.step += 1
    result["state"] = sm.state()
    return result
