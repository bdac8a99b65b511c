"""adaptive_stereo.utils.stereo_priority_queue.StereoPriorityQueue against the reference's own class, through the recorded trace
tests/golden/priority_queue_trace.json (tests/golden/make_golden_priority_queue.py): every return value and, after every
operation, the sorted (key, index) membership.  The trace's "unit_test" script is the reference's own unit test, recorded while
it ran on the reference's class.  Also the import paths that INTEGRATION.md promises."""
import json
import os

import pytest

from conftest import GOLDEN_DIR

TRACE = json.load(open(os.path.join(GOLDEN_DIR, "priority_queue_trace.json")))
CONFIGS = TRACE["configs"]
IDS = ["%s%d" % ("min" if c["min_heap"] else "max", c["max_size"]) for c in CONFIGS]


def members(q):
  return sorted([float(item[0]), int(item[1])] for item in q.buf)


def test_both_modules_import_by_the_reference_paths():
  from adaptive_stereo.utils.entropy import grayscale_shannon_entropy, gradient_shannon_entropy      # noqa: F401
  from adaptive_stereo.utils.stereo_priority_queue import StereoPriorityQueue                         # noqa: F401
  names = {}
  exec("from adaptive_stereo.utils.entropy import *", names)
  assert {"grayscale_shannon_entropy", "gradient_shannon_entropy"} <= set(names)


def test_trace_covers_what_it_should():
  unit = TRACE["unit_test"]["main"]
  assert len(unit) >= 10 and any(op["op"] == "pop" for op in unit) and any(not op["result"] for op in unit if op["op"] == "offer")
  assert [(c["max_size"], c["min_heap"]) for c in CONFIGS] == [(1, True), (1, False), (3, True), (3, False), (8, True), (8, False)]
  kinds = {}
  for c in CONFIGS:
    for op in c["main"] + c["popped_index"]:
      k = op.get("kind", "pop")
      kinds[k] = kinds.get(k, 0) + 1
  assert sum(kinds.values()) >= 300
  for k in ("grid", "worst", "below", "above", "member_index", "pop", "popped_index"):
    assert kinds.get(k, 0) > 0, k
  # an offer equal to the worst key is refused at capacity; its lower fp32 neighbour is kept
  ops = [op for c in CONFIGS for op in c["main"]]
  assert all(not op["result"] for op in ops if op.get("kind") in ("worst", "above"))
  assert any(op["result"] for op in ops if op.get("kind") == "below")


SCRIPTS = [(c, s) for s in ("main", "popped_index") for c in CONFIGS] + [(TRACE["unit_test"], "main")]
SCRIPT_IDS = ["%s-%s" % (s, i) for s in ("main", "popped_index") for i in IDS] + ["unit_test"]


@pytest.mark.parametrize("config,script", SCRIPTS, ids=SCRIPT_IDS)
def test_host_queue_replays_the_reference_trace(config, script):
  from adaptive_stereo.utils.stereo_priority_queue import StereoPriorityQueue
  q = StereoPriorityQueue(config["max_size"], min_heap=config["min_heap"])
  own_images = "images" not in config[script][0]            # the scripted offers name their images after the index
  for step, op in enumerate(config[script]):
    if op["op"] == "pop":
      item = q.pop()
      assert [float(item[0]), int(item[1])] == op["result"] and [item[2], item[3]] == op["images"], step
    else:
      left, right = ("L%d" % op["index"], "R%d" % op["index"]) if own_images else op["images"]
      got = q.add(left, right, op["value"], op["index"])
      assert got is op["result"], (step, op)
    assert members(q) == op["members"], (step, op)
    assert q.size() == len(op["members"])
    assert {m[1] for m in op["members"]} <= q.indices
    if own_images:
      for item in q.buf:
        assert item[2] == "L%d" % item[1] and item[3] == "R%d" % item[1]
    if q.size():
      sign = 1 if config["min_heap"] else -1
      assert q.average_value() == sum(sign * m[0] for m in op["members"]) / len(op["members"])


def test_max_heap_keeps_the_largest_values():
  from adaptive_stereo.utils.stereo_priority_queue import StereoPriorityQueue
  q = StereoPriorityQueue(2, min_heap=False)
  for i, v in enumerate((1.0, 5.0, 3.0, 5.0, 4.0)):
    q.add("l", "r", v, i)
  assert members(q) == [[-5.0, 1], [-5.0, 3]]
  assert q.average_value() == 5.0 and q.pop()[:2] == [-5.0, 1]
