"""adaptive_stereo.capture on its own: warm-up and capture on one side stream, the owner's capture origin, the put-back of
named state (also when the warm-up re-homes a tensor behind its name, as a StepPlan does with the BatchNorm counters), and
the static-input helpers.  Bodies are in-place adds on 16- and 1-element tensors: nothing here depends on a shape, and nothing
raises inside an open capture (the refusal of a nested capture is OnlineAdapter's and SupervisedTrainer's tests' business)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from adaptive_stereo import capture as cap
from adaptive_stereo.hip_ops import adjacent_or_cat

DEV = "cuda"


class _Owner(object):
  _capture_origin = None


def _bits(t):
  return t.detach().clone().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


class _Probe(object):
  """warm / body that add 1 to every tensor of ``tensors()`` and note, on the host, what they saw."""

  def __init__(self, tensors, owner):
    self.tensors, self.owner = tensors, owner
    self.warm_seen, self.body_seen = [], []

  def _run(self, seen):
    seen.append((torch.cuda.is_current_stream_capturing(), torch.cuda.current_stream().cuda_stream, self.owner._capture_origin))
    for t in self.tensors():
      t.add_(1)

  def warm(self):
    self._run(self.warm_seen)

  def body(self):
    self._run(self.body_seen)
    return "result"


@pytest.mark.parametrize("n", [1, 3])
def test_warm_up_runs_n_times_and_the_capture_records_one_body(n):
  x = torch.full((16,), 0.5, device=DEV)
  owner = _Owner()
  probe = _Probe(lambda: [x], owner)
  main = torch.cuda.current_stream().cuda_stream
  graph, result = cap.warm_up_and_capture(probe.warm, n, probe.body, owner=owner)
  torch.cuda.synchronize()
  assert result == "result" and len(probe.warm_seen) == n and len(probe.body_seen) == 1
  capturing, side, origin = probe.body_seen[0]
  assert capturing and origin == side and side != main            # the owner knows the capturing stream while it captures
  assert probe.warm_seen == [(False, side, None)] * n             # warm-up: same side stream, no capture open, no origin
  assert owner._capture_origin is None and not torch.cuda.is_current_stream_capturing()
  assert torch.equal(x, torch.full((16,), 0.5 + n, device=DEV))   # no put-back: n warm-up adds; the capture executed nothing
  for replays in (1, 2):
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(x, torch.full((16,), 0.5 + n + replays, device=DEV))


def test_put_back_restores_named_state_also_behind_a_re_homed_name():
  state = {"running": torch.linspace(-1.0, 2.0, 16, device=DEV), "counter": torch.tensor([7], dtype=torch.int64, device=DEV)}
  before = {name: _bits(t) for name, t in state.items()}
  first_counter = state["counter"]
  untouched = torch.zeros(1, device=DEV)           # changed by warm-up and body, not named: stays changed
  owner = _Owner()
  probe = _Probe(lambda: list(state.values()) + [untouched], owner)
  lookups = []

  def warm():
    if not probe.warm_seen:                         # the first warm-up step re-homes the counter: same name, another tensor
      state["counter"] = state["counter"].clone()
    probe.warm()

  def lookup():
    lookups.append(len(probe.warm_seen) + len(probe.body_seen))
    return dict(state)

  graph, _ = cap.warm_up_and_capture(warm, 2, probe.body, owner=owner, state=lookup)
  torch.cuda.synchronize()
  assert lookups == [0, 3]                          # once before the warm-up, once after the capture
  assert len(probe.warm_seen) == 2 and len(probe.body_seen) == 1 and probe.body_seen[0][0]
  assert state["counter"] is not first_counter
  for name, t in state.items():
    assert torch.equal(_bits(t), before[name]), name
  assert float(untouched) == 2.0
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(state["running"], torch.linspace(-1.0, 2.0, 16, device=DEV) + 1) and int(state["counter"]) == 8
  assert int(first_counter) == 7 and float(untouched) == 3.0      # the graph updates the re-homed tensor, not the old one


def test_two_graphs_on_one_warm_up_stream_share_a_pool():
  """The two-graph data-parallel step: warm_up once, capture_graph twice, the second with the first's pool."""
  x = torch.zeros(1, device=DEV)
  owner = _Owner()
  probe = _Probe(lambda: [x], owner)
  side = cap.warm_up(probe.warm, 1)
  g1, _ = cap.capture_graph(side, probe.body, owner=owner)
  g2, _ = cap.capture_graph(side, probe.body, owner=owner, pool=g1.pool())
  assert [s[:2] for s in probe.body_seen] == [(True, side.cuda_stream)] * 2 and owner._capture_origin is None
  assert g2.pool() == g1.pool()
  g1.replay(); g2.replay()
  torch.cuda.synchronize()
  assert float(x) == 3.0


def test_copy_unless_same_compares_the_address():
  buf = torch.arange(32.0, device=DEV)
  dst, overlapping = buf[:16], buf[::2]             # same address, other values: a copy would change dst (or be refused)
  assert overlapping.data_ptr() == dst.data_ptr()
  cap.copy_unless_same(dst, overlapping)
  cap.copy_unless_same(dst, dst)
  assert torch.equal(dst, torch.arange(16.0, device=DEV))
  cap.copy_unless_same(dst, buf[16:])               # same storage, another address: copied
  assert torch.equal(dst, torch.arange(16.0, 32.0, device=DEV))
  sentinel = torch.full((16,), -3.0, device=DEV)
  cap.copy_unless_same(dst, sentinel)
  assert torch.equal(dst, sentinel) and torch.equal(buf[16:], torch.arange(16.0, 32.0, device=DEV))


def test_static_pair_is_two_adjacent_halves_of_one_buffer():
  left = torch.arange(16.0, device=DEV).reshape(2, 1, 2, 4)
  right = left + 100.0
  sl, sr = cap.static_pair(left, right)
  assert torch.equal(sl, left) and torch.equal(sr, right)
  assert sl.data_ptr() not in (left.data_ptr(), right.data_ptr())
  assert sl.untyped_storage().data_ptr() == sr.untyped_storage().data_ptr()
  assert sr.data_ptr() == sl.data_ptr() + sl.numel() * sl.element_size()
  both = adjacent_or_cat(sl, sr)                    # what the pair pass does with them: a view, no copy
  assert both.data_ptr() == sl.data_ptr() and torch.equal(both, torch.cat([left, right]))
