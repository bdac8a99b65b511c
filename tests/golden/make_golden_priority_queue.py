"""Generates tests/golden/priority_queue_trace.json by driving the REFERENCE's own StereoPriorityQueue.

Run in the build container only (needs /root/reference; the GPU box never has it):

    python tests/golden/make_golden_priority_queue.py

Per configuration (max_size 1, 3 and 8, min and max heap) two scripts of operations, and one more for the whole file, each recorded with what the reference
returned and the queue's membership afterwards, sorted [(key, index)] (key = value or -value, as the reference stores it):

  main           offers and pops.  Values are exactly representable in fp32 and come from a coarse grid (so ties on the key with
                 different indices are common), from the worst member's key itself, and from its two fp32 neighbours; indices
                 repeat those of members and of evicted items.  An index that was popped is never offered again.
  popped_index   a short script that does offer popped indices again: the reference's pop() leaves the index in its `indices`
                 set, so the offer is refused.  The host class keeps that; the device class documents that it does not, and is
                 not replayed on this script.
  unit_test      (one configuration) the reference's own test/test_stereo_priority_queue.py, run as it is on a subclass of
                 the reference's class that writes down every add() and pop() with its result and the membership after it.

Strings stand in as images.  No reference source text is stored — only the operations and their results.
"""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference"
sys.path.insert(0, REFERENCE)
from adaptive_stereo.utils import stereo_priority_queue as ref_pq                   # noqa: E402

assert ref_pq.__file__.startswith(REFERENCE)

CONFIGS = [(cap, min_heap) for cap in (1, 3, 8) for min_heap in (True, False)]
MAIN_OPS, POPPED_OPS = 70, 24


def f32(x):
  return float(np.float32(x))


def membership(q):
  return sorted([float(item[0]), int(item[1])] for item in q.buf)


def worst_key(q):
  return max((item[0], item[1]) for item in q.buf)[0]


def script(cap, min_heap, n_ops, seed, reoffer_popped):
  rng = random.Random(seed)
  q = ref_pq.StereoPriorityQueue(cap, min_heap=min_heap)
  sign = 1.0 if min_heap else -1.0
  popped, ops = set(), []
  kinds = dict(grid=0, worst=0, below=0, above=0, member_index=0, pop=0, popped_index=0)
  for step in range(n_ops):
    full = q.size() == cap
    kind = rng.choice(("grid", "grid", "grid", "worst", "below", "above", "member_index", "pop"))
    if kind in ("worst", "below", "above") and not full:
      kind = "grid"
    if kind in ("pop", "member_index") and q.size() == 0:
      kind = "grid"
    if reoffer_popped and popped and step % 3 == 2:
      kind = "popped_index"
    kinds[kind] += 1
    if kind == "pop":
      item = q.pop()
      popped.add(item[1])
      ops.append({"op": "pop", "result": [float(item[0]), int(item[1])], "images": [item[2], item[3]],
                  "members": membership(q)})
      continue
    if kind == "worst":
      key = worst_key(q)
    elif kind == "below":
      key = f32(np.nextafter(np.float32(worst_key(q)), np.float32(-np.inf)))
    elif kind == "above":
      key = f32(np.nextafter(np.float32(worst_key(q)), np.float32(np.inf)))
    else:
      key = rng.randrange(-6, 7) * 0.25                    # 13 values: ties are common
    value = sign * key
    assert f32(value) == value
    if kind == "member_index":
      index = rng.choice(membership(q))[1]
    elif kind == "popped_index":
      index = rng.choice(sorted(popped))
    else:
      index = rng.choice([i for i in range(-2, 4 * cap + 8) if i not in popped])
    result = q.add("L%d" % index, "R%d" % index, value, index)
    ops.append({"op": "offer", "value": value, "index": index, "kind": kind, "result": bool(result),
                "members": membership(q)})
  return ops, kinds


def unit_test_script():
  """Runs the reference's unit test file on a recording subclass of its class: (max_size, min_heap, operations)."""
  import importlib.util
  import unittest
  sys.path.insert(0, os.path.join(REFERENCE, "adaptive_stereo"))          # the test file imports `utils.stereo_priority_queue`
  spec = importlib.util.spec_from_file_location("reference_test_pq", os.path.join(REFERENCE, "test", "test_stereo_priority_queue.py"))
  module = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(module)
  made, ops = [], []

  class Recorder(module.StereoPriorityQueue):
    def __init__(self, max_size, min_heap=True):
      super().__init__(max_size, min_heap=min_heap)
      made.append((max_size, min_heap))

    def add(self, img_l, img_r, value, index):
      result = super().add(img_l, img_r, value, index)
      ops.append({"op": "offer", "value": float(value), "index": int(index), "kind": "unit_test", "images": [img_l, img_r],
                  "result": bool(result), "members": membership(self)})
      return result

    def pop(self):
      item = super().pop()
      ops.append({"op": "pop", "result": [float(item[0]), int(item[1])], "images": [item[2], item[3]],
                  "members": membership(self)})
      return item

  module.StereoPriorityQueue = Recorder
  result = unittest.TestResult()
  unittest.TestLoader().loadTestsFromModule(module).run(result)
  assert result.wasSuccessful() and result.testsRun >= 1 and len(made) == 1, (result.errors, result.failures, made)
  return made[0][0], made[0][1], ops


def main():
  out = {"what": "operations on the reference's StereoPriorityQueue with its return values and sorted (key, index) membership",
         "configs": []}
  total = {}
  for n, (cap, min_heap) in enumerate(CONFIGS):
    main_ops, k1 = script(cap, min_heap, MAIN_OPS, 100 + n, False)
    popped_ops, k2 = script(cap, min_heap, POPPED_OPS, 200 + n, True)
    for k in (k1, k2):
      for name, c in k.items():
        total[name] = total.get(name, 0) + c
    out["configs"].append({"max_size": cap, "min_heap": min_heap, "main": main_ops, "popped_index": popped_ops})
  assert all(c > 0 for c in total.values()), total
  cap, min_heap, ops = unit_test_script()
  out["unit_test"] = {"max_size": cap, "min_heap": min_heap, "main": ops}
  path = os.path.join(HERE, "priority_queue_trace.json")
  with open(path, "w") as f:
    json.dump(out, f, indent=None, separators=(",", ":"), sort_keys=True)
    f.write("\n")
  print("%s: %.1f KB, operations by kind %s, unit test %d operations" % (path, os.path.getsize(path) / 1e3, total, len(ops)))


if __name__ == "__main__":
  main()
