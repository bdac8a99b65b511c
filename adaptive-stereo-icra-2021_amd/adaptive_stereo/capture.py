"""Capturing a step into a hipGraph: the rules every captured step here follows, in one place.

Each rule stands for a crash or wrong bits seen on ROCm 7.2:
  * warm-up and capture run on the SAME side stream: the free lists of hip_ops.PclPool are per stream, so only then does the
    capture reuse the warm-up's buffers instead of allocating;
  * no capture inside a capture: a fork from an already forked stream crashes hipStreamEndCapture.  refuse_nested() raises
    before anything is issued, and while a capture of ours is open its owner's ``_capture_origin`` holds the capturing stream's
    handle, which is how OnlineAdapter._features_two_streams tells its own capture (fork) from a foreign one (one stream);
  * capture_error_mode="thread_local": the process-group watchdog thread polls events while a capture is open; only this
    thread's calls have to be capture-safe.
Warm-up steps are real steps.  Their number is the caller's (a StepPlan records on its first step and runs from the second), and
a caller whose warm-up must leave no trace names the tensors to put back (``state``).
"""
import torch


def refuse_nested(what):
  if torch.cuda.is_current_stream_capturing():
    raise RuntimeError("%s: the current stream is already being captured; a capture inside a capture "
                       "(and the stream fork it implies) crashes hipStreamEndCapture on ROCm 7.2 — capture from an "
                       "ordinary stream, or call step()/infer() inside your own capture (they then run the "
                       "one-stream order)" % what)


def warm_up(warm, n):
  """Runs ``warm()`` n times on a fresh side stream, ordered behind the current stream, and waits for it; returns the stream."""
  current = torch.cuda.current_stream()
  side = torch.cuda.Stream()
  side.wait_stream(current)
  with torch.cuda.stream(side):
    for _ in range(n):
      warm()
  current.wait_stream(side)
  torch.cuda.synchronize()
  return side


def capture_graph(side, body, owner=None, pool=None):
  """Captures ``body()`` on ``side`` (the warm-up's stream) -> (graph, body's result).  ``owner._capture_origin`` is the stream's
  handle for exactly as long as the capture is open.  ``pool``: the memory pool of an earlier graph of the same step."""
  graph = torch.cuda.CUDAGraph()
  if owner is not None:
    owner._capture_origin = side.cuda_stream
  try:
    with torch.cuda.graph(graph, pool=pool, stream=side, capture_error_mode="thread_local"):
      result = body()
  finally:
    if owner is not None:
      owner._capture_origin = None
  return graph, result


def warm_up_and_capture(warm, n, body, owner=None, state=None):
  """warm_up + capture_graph.  ``state()`` -> {name: tensor} of what the warm-up must not change: cloned before it, copied back by
  name after the capture.  Looked up anew then: a StepPlan built during the warm-up re-homes the BatchNorm batch counters (same
  names, other tensors), and the put-back must reach the tensors the graph updates."""
  saved = None if state is None else {name: t.clone() for name, t in state().items()}
  graph, result = capture_graph(warm_up(warm, n), body, owner)
  if saved is not None:
    with torch.no_grad():
      for name, t in state().items():
        t.copy_(saved[name])
  return graph, result


def static_pair(left, right):
  """Copies of both images as the two halves of ONE buffer: the pair pass of the feature extractor then needs no concatenation."""
  pair = torch.cat([left, right])
  return pair[:left.shape[0]], pair[left.shape[0]:]


def copy_unless_same(dst, src):
  """``src`` into the static buffer ``dst``, unless the caller filled that very buffer (graph_inputs())."""
  if src.data_ptr() != dst.data_ptr():
    dst.copy_(src)
