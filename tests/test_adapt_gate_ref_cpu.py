"""tests/adapt_gate_ref.py against the host classes it restates: StateMachine.add_to_ovs / StereoReservoir.add and the decisions
of AdaptationLoop.process, with random.randint patched to 1 + min(int(u * b), b - 1) on the step's own u."""
import random

import torch

from adapt_gate_ref import GateRef, randint_from_uniform, f32
from adaptive_stereo.control import StateMachine, State
from adaptive_stereo.utils import stereo_reservoir


def _host_step(sm, fcs, loss, batch_idx, threshold, gate_enabled):
  """The decisions of AdaptationLoop.process (control.py) around a given forward result."""
  adapting = sm.state() == State.IN_PROGRESS
  novel, did_add = False, False
  if gate_enabled:
    novel = float(fcs) < threshold
    if novel:
      did_add = bool(sm.add_to_ovs(torch.zeros(1), torch.zeros(1), loss, batch_idx))
  updated = sm.state() == State.IN_PROGRESS and adapting and not did_add
  return novel, did_add, updated


def _run(capacity, steps, seed, index_range, monkeypatch):
  rng = random.Random(seed)
  sm = StateMachine(State.IN_PROGRESS, ovs_buffer_size=capacity)
  ref = GateRef(capacity)
  cur = {}
  monkeypatch.setattr(stereo_reservoir.random, "randint", lambda a, b: randint_from_uniform(cur["u"], b))
  threshold = 10.0
  seen = dict(non_novel=0, append=0, duplicate=0, replace=0, no_replace=0, done=0, gate_off=0)
  adds = updates = 0
  for step in range(steps):
    fcs = f32(rng.choice((threshold, threshold - 1e-3, threshold + 1e-3, rng.uniform(0, 20), float("nan"), float("-inf"))))
    loss = f32(rng.uniform(0.0, 2.0))
    idx = rng.randrange(index_range)
    u = rng.choice((0.0, 1.0 - 2.0 ** -53, rng.random(), rng.random() * capacity / max(1, ref.offers + 1)))
    gate_enabled = rng.random() > 0.05
    if rng.random() < 0.05:
      sm.current_state = State.DONE                     # a finished machine: no update, any offer restarts it
    adapting = sm.state() == State.IN_PROGRESS
    cur["u"] = u
    full_before, size_before = len(sm.ovs.buf) == capacity, len(sm.ovs.buf)
    dup = idx in sm.ovs.indices
    novel, did_add, updated = _host_step(sm, fcs, loss, idx, threshold, gate_enabled)
    r_novel, r_slot, r_update = ref.step(fcs, loss, idx, u, threshold, gate_enabled, adapting)
    adds += did_add; updates += updated
    assert (int(novel), int(did_add), int(updated)) == (r_novel, int(r_slot >= 0), r_update), step
    assert (len(sm.ovs.buf), sm.ovs.i, adds, updates) == ref.state(), step
    assert sm.ovs.indices == set(ref.indices[:ref.size]) and len(sm.ovs.indices) == ref.size
    assert [e[0] for e in sm.ovs.buf] == ref.values[:ref.size], step
    if novel:
      assert sm.state() == State.IN_PROGRESS            # restarted by the offer
    seen["non_novel"] += not novel and gate_enabled
    seen["gate_off"] += not gate_enabled
    seen["done"] += not adapting
    seen["duplicate"] += novel and dup
    seen["append"] += novel and not dup and not full_before
    seen["replace"] += novel and not dup and full_before and did_add
    seen["no_replace"] += novel and not dup and full_before and not did_add
    if novel and not dup and not full_before:
      assert r_slot == size_before
  return seen


def test_gate_ref_equals_state_machine_and_reservoir(monkeypatch):
  total = {}
  for capacity, steps, seed, index_range in ((1, 600, 1, 4), (3, 1500, 2, 12), (8, 2500, 3, 400)):
    seen = _run(capacity, steps, seed, index_range, monkeypatch)
    assert all(v > 0 for v in seen.values()), (capacity, seen)
    for k, v in seen.items():
      total[k] = total.get(k, 0) + v
  assert total["replace"] > 20 and total["no_replace"] > 20 and total["duplicate"] > 20


def test_randint_from_uniform_covers_the_range():
  assert randint_from_uniform(0.0, 7) == 1 and randint_from_uniform(1.0 - 2.0 ** -53, 7) == 7
  assert randint_from_uniform(1.0 - 2.0 ** -53, (1 << 24) + 5) == (1 << 24) + 5
  assert sorted({randint_from_uniform(i / 70.0, 7) for i in range(70)}) == [1, 2, 3, 4, 5, 6, 7]
