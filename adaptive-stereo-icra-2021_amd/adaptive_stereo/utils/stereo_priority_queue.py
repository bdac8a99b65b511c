"""A buffer that keeps the K most (or least) novel stereo pairs of a stream: the alternative to the reservoir.

Reference: adaptive_stereo/utils/stereo_priority_queue.py.  Two classes with the same membership rules:

  StereoPriorityQueue   host-side control logic with the reference's surface; the entries are whatever the caller stores.
  DevicePriorityQueue   the pairs, keys and bookkeeping in device memory, decided by as_pq_offer and filled by
                        as_reservoir_store (csrc/adapt_gate.hip): an offer is two launches and no read-back, so it sits in a
                        captured step beside ood.FcsCollector.

The rules.  key = value for a min heap, -value for a max heap.  An index already present is refused.  Below max_size the item is
always kept.  At max_size the worst member is the maximum by (key, index), and the offer replaces it only when its key is
strictly smaller.  pop() removes and returns the minimum by (key, index).

One thing differs between the two on purpose.  The reference's pop() leaves the popped item's index in `indices`, so that index
stays refused for ever; StereoPriorityQueue keeps that (callers may rely on `indices`).  DevicePriorityQueue looks for
duplicates among its members only, so an index may be offered again once it has been popped.
"""
import torch

from .. import _native as nat
from ..collect import gpu_device


class StereoPriorityQueue(object):
  def __init__(self, max_size, min_heap=True):
    """max_size: how many items the buffer holds at most.  min_heap: keep the smallest values (True) or the largest (False)."""
    self.max_size = max_size
    self.min_heap = min_heap
    self.multiplier = 1 if min_heap else -1
    self.buf = []                 # [key, index, img_l, img_r], ascending by (key, index)
    self.indices = set()

  @staticmethod
  def _order(item):
    return (item[0], item[1])

  def _insert(self, item):
    at = len(self.buf)
    while at > 0 and self._order(self.buf[at - 1]) > self._order(item):
      at -= 1
    self.buf.insert(at, item)
    self.indices.add(item[1])

  def add(self, img_l, img_r, value, index):
    """Offers an item; returns True when it was stored."""
    if index in self.indices:
      return False
    key = self.multiplier * value
    if len(self.buf) >= self.max_size:
      if not self.buf or not key < self.buf[-1][0]:
        return False
      self.indices.remove(self.buf.pop()[1])
    self._insert([key, index, img_l, img_r])
    return True

  def size(self):
    return len(self.buf)

  def pop(self):
    """Removes and returns the best item, [key, index, img_l, img_r]; its index stays in `indices` (see the module text)."""
    return self.buf.pop(0)

  def average_value(self):
    return sum(self.multiplier * item[0] for item in self.buf) / len(self.buf)


class DevicePriorityQueue(object):
  """StereoPriorityQueue's membership on the device (include/adaptive_stereo_hip.h, as_pq_offer, for the exact rules; keys are
  fp32 and a NaN value is always refused).

  state    int64 [size, offers, adds]      indices int32 [max_size]      keys fp32 [max_size]
  left / right  fp32 [max_size, ...], allocated when the first pair shows its shape (or by allocate)
  out_slot int32 [1]: the row the last offer went to, or -1

  offer() only enqueues.  size(), average_value(), items() and pop() read the device (a host synchronisation)."""

  def __init__(self, max_size, min_heap=True, device="cuda"):
    if max_size < 1:
      raise ValueError("DevicePriorityQueue: max_size must be at least 1")
    dev = gpu_device("DevicePriorityQueue", device)
    self.max_size = int(max_size)
    self.min_heap = bool(min_heap)
    self.multiplier = 1 if min_heap else -1
    self.state = torch.zeros(3, dtype=torch.int64, device=dev)
    self.indices = torch.zeros(self.max_size, dtype=torch.int32, device=dev)
    self.keys = torch.zeros(self.max_size, dtype=torch.float32, device=dev)
    self.out_slot = torch.full((1,), -1, dtype=torch.int32, device=dev)
    self._value = torch.zeros(1, dtype=torch.float32, device=dev)       # cells for python numbers
    self._index = torch.zeros(1, dtype=torch.int32, device=dev)
    self.left = self.right = None

  def allocate(self, like):
    if self.left is None:
      self.left = torch.zeros((self.max_size,) + tuple(like.shape), dtype=torch.float32, device=self.state.device)
      self.right = torch.zeros_like(self.left)
    elif tuple(self.left.shape[1:]) != tuple(like.shape):
      raise ValueError("DevicePriorityQueue: pairs of %s, allocated for %s" % (tuple(like.shape), tuple(self.left.shape[1:])))

  def _cell(self, x, cell, what):
    if torch.is_tensor(x):
      if not x.is_cuda or x.device != cell.device or x.dtype != cell.dtype or x.numel() != 1:
        raise RuntimeError("DevicePriorityQueue.offer: %s must be one %s element on %s, or a python number (got %s %s on %s)"
                           % (what, cell.dtype, cell.device, tuple(x.shape), x.dtype, x.device))
      return x
    if torch.cuda.is_current_stream_capturing():
      raise RuntimeError("DevicePriorityQueue.offer: a python %s cannot change between replays; pass a device tensor inside a "
                         "capture" % what)
    cell.fill_(x)
    return cell

  def offer(self, left, right, value, index):
    """Offers a pair: `value` (fp32) and `index` (int32) are one-element device tensors, or python numbers (copied to the
    queue's own cells; not inside a capture).  left / right: contiguous fp32 device tensors of one shape.  Two launches, no
    host read; out_slot says where the pair went."""
    nat.require_gpu(left, right)
    if left.shape != right.shape or left.dtype != torch.float32 or right.dtype != torch.float32 or \
       not left.is_contiguous() or not right.is_contiguous() or left.device != self.state.device or left.numel() == 0:
      raise RuntimeError("DevicePriorityQueue.offer: left and right must be contiguous fp32 tensors of one shape on %s"
                         % self.state.device)
    if self.left is None and torch.cuda.is_current_stream_capturing():
      raise RuntimeError("DevicePriorityQueue.offer: call allocate(like) before the capture")
    self.allocate(left)
    value = self._cell(value, self._value, "value")
    index = self._cell(index, self._index, "index")
    with torch.cuda.device(self.state.device):
      nat.call("as_pq_offer", nat.ptr(value), nat.ptr(index), self.max_size, int(self.min_heap), nat.ptr(self.state),
               nat.ptr(self.indices), nat.ptr(self.keys), nat.ptr(self.out_slot), nat.stream())
      nat.call("as_reservoir_store", nat.ptr(left), nat.ptr(right), left.numel(), nat.ptr(self.out_slot), self.max_size,
               nat.ptr(self.left), nat.ptr(self.right), nat.stream())

  # -- host side: each of these synchronises ----------------------------------------------------------
  def counters(self):
    """(size, offers, adds) as python ints."""
    return tuple(int(v) for v in self.state.cpu().tolist())

  def size(self):
    return int(self.state[0])

  def _members(self):
    n = self.size()
    keys, idx = self.keys[:n].cpu().tolist(), self.indices[:n].cpu().tolist()
    return sorted(zip(keys, idx, range(n)))

  def average_value(self):
    vals = [self.multiplier * k for k, _, _ in self._members()]
    return sum(vals) / len(vals)

  def items(self):
    """[(key, index, left, right)] ascending by (key, index); left and right are views of the queue's rows."""
    return [(k, i, self.left[row], self.right[row]) for k, i, row in self._members()]

  def pop(self):
    """Removes and returns the best member, [key, index, left, right] (clones); the last row moves into its place."""
    members = self._members()
    if not members:
      raise IndexError("pop from an empty DevicePriorityQueue")
    key, index, row = members[0]
    out = [key, index, self.left[row].clone(), self.right[row].clone()]
    last = len(members) - 1
    if row != last:
      self.left[row].copy_(self.left[last])
      self.right[row].copy_(self.right[last])
      self.keys[row:row + 1].copy_(self.keys[last:last + 1])
      self.indices[row:row + 1].copy_(self.indices[last:last + 1])
    self.state[0:1].sub_(1)
    return out
