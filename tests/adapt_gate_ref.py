"""Plain-Python restatement of as_adapt_gate (include/adaptive_stereo_hip.h): the per-step decisions of
control.AdaptationLoop.process plus utils.stereo_reservoir.StereoReservoir.add, with random.randint(1, offers) drawn from one
uniform double as 1 + min(int(u * offers), offers - 1).  tests/test_adapt_gate_ref_cpu.py holds it to the host classes,
tests/test_gpu_adapt_gate.py holds the kernel to it."""
import struct


def f32(x):
  """x rounded to binary32, as a python float (NaN and infinities pass)."""
  return struct.unpack("<f", struct.pack("<f", x))[0]


def randint_from_uniform(u, b):
  """random.randint(1, b) from a uniform u in [0, 1)."""
  return 1 + min(int(u * b), b - 1)


class GateRef(object):
  def __init__(self, capacity):
    self.capacity = capacity
    self.size = self.offers = self.adds = self.updates = 0
    self.indices = [0] * capacity
    self.values = [0.0] * capacity

  def step(self, fcs_smoothed, loss, batch_idx, u, threshold, gate_enabled=True, adapting=True):
    """-> (novel, slot, update).  fcs_smoothed and loss are binary32 values, threshold and u doubles."""
    novel = bool(gate_enabled) and (float(fcs_smoothed) < threshold)          # strict: NaN is never novel
    slot = -1
    if novel:
      self.offers += 1
      if batch_idx not in self.indices[:self.size]:
        if self.size < self.capacity:
          slot = self.size
          self.indices[self.size] = batch_idx
          self.size += 1
        else:
          r = randint_from_uniform(u, self.offers)
          if r <= self.capacity:
            slot = r - 1
      if slot >= 0:
        self.values[slot] = f32(loss)
        self.adds += 1
    update = bool(adapting) and slot < 0
    self.updates += int(update)
    return int(novel), slot, int(update)

  def state(self):
    return (self.size, self.offers, self.adds, self.updates)
