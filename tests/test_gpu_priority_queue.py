"""as_pq_offer (csrc/adapt_gate.hip) and adaptive_stereo.utils.stereo_priority_queue.DevicePriorityQueue on the GPU.

The reference is the reference's own class through the recorded trace tests/golden/priority_queue_trace.json (its "main"
scripts; the "popped_index" scripts pin the one point where the device class differs on purpose, see the module text), and the
host class StereoPriorityQueue, which tests/test_priority_queue_cpu.py holds to the same trace.  Keys are fp32 and every value
of the trace is exactly representable, so membership is compared for equality.
"""
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from adaptive_stereo import _native as nat
from adaptive_stereo.utils.stereo_priority_queue import DevicePriorityQueue, StereoPriorityQueue
from conftest import GOLDEN_DIR

DEV = "cuda:0"
SHAPE = (3, 5, 7)
GUARD = 123456.0
TRACE = json.load(open(os.path.join(GOLDEN_DIR, "priority_queue_trace.json")))
CONFIGS = TRACE["configs"]
IDS = ["%s%d" % ("min" if c["min_heap"] else "max", c["max_size"]) for c in CONFIGS]


def image(index, side):
  return torch.full(SHAPE, float(index) + (0.5 if side else 0.0), device=DEV)


def guarded(q):
  """Puts the queue's rows between two guard rows: (whole_left, whole_right)."""
  whole = [torch.full((q.max_size + 2,) + SHAPE, GUARD, device=DEV) for _ in range(2)]
  q.left, q.right = whole[0][1:-1], whole[1][1:-1]
  q.left.zero_(); q.right.zero_()
  return whole


def members(q):
  return [[float(k), int(i)] for k, i, _, _ in q.items()]


def snapshot(q, whole):
  return [t.clone() for t in (whole[0], whole[1], q.keys, q.indices)]


def assert_rows_hold_their_images(q, whole):
  for key, index, left, right in q.items():
    assert bool((left == float(index)).all()) and bool((right == float(index) + 0.5).all()), index
  for w in whole:
    assert bool((w[0] == GUARD).all()) and bool((w[-1] == GUARD).all()), "a guard row was written"


@pytest.mark.parametrize("config", CONFIGS, ids=IDS)
def test_device_queue_replays_the_reference_trace(config):
  q = DevicePriorityQueue(config["max_size"], min_heap=config["min_heap"], device=DEV)
  whole = guarded(q)
  offers = adds = 0
  for step, op in enumerate(config["main"]):
    if op["op"] == "pop":
      item = q.pop()
      assert [float(item[0]), int(item[1])] == op["result"], step
      assert bool((item[2] == float(item[1])).all()) and bool((item[3] == float(item[1]) + 0.5).all())
    else:
      before = snapshot(q, whole)
      q.offer(image(op["index"], 0), image(op["index"], 1), op["value"], op["index"])
      slot = int(q.out_slot[0])
      offers += 1
      adds += op["result"]
      assert (slot >= 0) is op["result"], (step, op, slot)
      if not op["result"]:
        assert slot == -1
        for a, b in zip(before, snapshot(q, whole)):
          assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a refused offer changed a byte"
    assert members(q) == op["members"], (step, op)
    assert q.size() == len(op["members"])
    assert_rows_hold_their_images(q, whole)
  assert q.counters() == (len(config["main"][-1]["members"]), offers, adds)


def test_nan_is_refused_full_or_not():
  for min_heap in (True, False):
    q = DevicePriorityQueue(2, min_heap=min_heap, device=DEV)
    whole = guarded(q)
    q.offer(image(0, 0), image(0, 1), float("nan"), 0)
    assert int(q.out_slot[0]) == -1 and q.size() == 0
    q.offer(image(1, 0), image(1, 1), 1.0, 1)
    q.offer(image(2, 0), image(2, 1), 2.0, 2)
    before = snapshot(q, whole)
    q.offer(image(3, 0), image(3, 1), float("nan"), 3)
    assert int(q.out_slot[0]) == -1 and q.counters() == (2, 4, 2)
    for a, b in zip(before, snapshot(q, whole)):
      assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    q.offer(image(4, 0), image(4, 1), float("-inf") if min_heap else float("inf"), 4)      # infinities are ordinary keys
    assert int(q.out_slot[0]) >= 0 and members(q)[0] == [float("-inf"), 4]
    assert q.average_value() == (float("-inf") if min_heap else float("inf"))


def random_offers(n, seed):
  rng = random.Random(seed)
  grid = [float(np.float32(x)) for x in (0.1, 0.1 + 2 ** -24, 0.3, 0.7, -0.2, 5.0, 5.0, 0.0, -0.0)]
  return [(rng.choice(grid) if rng.random() < 0.6 else float(np.float32(rng.uniform(-1, 6))), rng.randrange(0, 60))
          for _ in range(n)]


@pytest.mark.parametrize("min_heap", [True, False])
def test_equals_the_host_class_on_random_offers_with_ties(min_heap):
  host = StereoPriorityQueue(5, min_heap=min_heap)
  q = DevicePriorityQueue(5, min_heap=min_heap, device=DEV)
  whole = guarded(q)
  slots = []
  for value, index in random_offers(200, 9):
    kept = host.add("l", "r", value, index)
    q.offer(image(index, 0), image(index, 1), value, index)
    slots.append((kept, q.out_slot.clone()))
  got = torch.cat([s for _, s in slots]).cpu().tolist()
  assert [k for k, _ in slots] == [s >= 0 for s in got]
  assert 5 < sum(s >= 0 for s in got) < 200               # the script fills the queue and replaces members, and refuses most
  assert members(q) == sorted([float(item[0]), int(item[1])] for item in host.buf)
  assert q.average_value() == host.average_value()
  assert_rows_hold_their_images(q, whole)


def test_captured_offer_replayed_with_new_device_scalars_equals_eager_offers():
  offers = random_offers(40, 3)
  eager = DevicePriorityQueue(4, device=DEV)
  eager.allocate(image(0, 0))
  for value, index in offers:
    eager.offer(image(index, 0), image(index, 1), value, index)

  q = DevicePriorityQueue(4, device=DEV)
  left, right = image(0, 0), image(0, 1)
  value = torch.zeros(1, device=DEV)
  index = torch.zeros(1, dtype=torch.int32, device=DEV)
  q.allocate(left)
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    q.offer(left, right, value, index)                     # warm-up outside the capture
  torch.cuda.synchronize()
  q.state.zero_(); q.keys.zero_(); q.indices.zero_(); q.left.zero_(); q.right.zero_()
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):     # one stream: a linear graph
    q.offer(left, right, value, index)
    with pytest.raises(RuntimeError, match="device tensor"):
      q.offer(left, right, 1.0, index)
  for v, i in offers:
    left.fill_(float(i)); right.fill_(float(i) + 0.5); value.fill_(v); index.fill_(i)
    graph.replay()
  torch.cuda.synchronize()
  assert q.counters() == eager.counters()
  assert torch.equal(q.keys, eager.keys) and torch.equal(q.indices, eager.indices)
  assert torch.equal(q.left, eager.left) and torch.equal(q.right, eager.right)


def test_argument_errors():
  q = DevicePriorityQueue(2, device=DEV)
  with pytest.raises(RuntimeError, match="no CPU path"):
    q.offer(torch.zeros(SHAPE), torch.zeros(SHAPE), 1.0, 1)
  with pytest.raises(RuntimeError, match="one shape"):
    q.offer(image(0, 0), image(0, 1)[:2], 1.0, 1)
  q.offer(image(0, 0), image(0, 1), 1.0, 1)
  with pytest.raises(ValueError, match="allocated for"):
    q.offer(torch.zeros(2, 2, device=DEV), torch.zeros(2, 2, device=DEV), 1.0, 2)
  with pytest.raises(RuntimeError, match="no CPU path"):
    DevicePriorityQueue(2, device="cpu")
  with pytest.raises(IndexError):
    DevicePriorityQueue(2, device=DEV).pop()
  lib = nat.load()
  assert lib.as_pq_offer(None, None, 1, 1, None, None, None, None, nat.stream()) != 0
  assert lib.as_pq_offer(nat.ptr(q._value), nat.ptr(q._index), 0, 1, nat.ptr(q.state), nat.ptr(q.indices), nat.ptr(q.keys),
                         nat.ptr(q.out_slot), nat.stream()) != 0
