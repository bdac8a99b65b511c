"""csrc/adapt_gate.hip and the gated clip + Adam of csrc/optim.hip: the gate kernel against tests/adapt_gate_ref.py word by word,
the reservoir store between guard floats, the gated optimizer bit for bit against the ungated entry points."""
import math
import random
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from adapt_gate_ref import GateRef, f32
from adaptive_stereo import _native as nat
from adaptive_stereo.adaptation import FlatArena, FusedClipAdam
from adaptive_stereo.control import DeviceReservoir

DEV = "cuda:0"
U_LAST = math.nextafter(1.0, 0.0)


def _f32_next(x, towards):
  return float(np.nextafter(np.float32(x), np.float32(towards)))


class _Gate(object):
  """A DeviceReservoir and its reference, stepped together and compared after every step."""

  def __init__(self, capacity):
    self.dev, self.ref = DeviceReservoir(capacity, DEV), GateRef(capacity)
    self.fcs = torch.zeros(1, dtype=torch.float32, device=DEV)
    self.loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    self.idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    self.u = torch.zeros(1, dtype=torch.float64, device=DEV)
    self.steps = 0

  def set_offers(self, offers):
    self.dev.state[1] = offers
    self.ref.offers = offers

  def step(self, fcs, loss, idx, u, threshold, gate_enabled=True, adapting=True):
    self.fcs.fill_(fcs); self.loss.fill_(loss); self.idx.fill_(idx); self.u.fill_(u)
    self.dev.gate(self.fcs, self.loss, self.idx, self.u, threshold, gate_enabled, adapting)
    exp = self.ref.step(f32(fcs), f32(loss), idx, u, threshold, gate_enabled, adapting)
    got = tuple(self.dev.out3.cpu().tolist())
    where = "step %d (fcs %r, idx %d, u %r)" % (self.steps, fcs, idx, u)
    assert got == exp, where
    assert self.dev.counters() == self.ref.state(), where
    assert self.dev.indices.cpu().tolist() == self.ref.indices, where
    vals = self.dev.values.cpu().numpy()
    assert vals.tobytes() == np.asarray(self.ref.values, dtype=np.float32).tobytes(), where
    self.steps += 1
    return exp


@pytest.mark.parametrize("threshold", [15.0, 0.1])
def test_gate_kernel_threshold_edges(threshold):
  """fcs == threshold and its binary32 neighbours (threshold 0.1 is no binary32 number: float32(0.1) lies above it), NaN, -inf,
  +inf; the comparison is strict and in double."""
  g = _Gate(8)
  t32 = f32(threshold)
  below, above = _f32_next(t32, -np.inf), _f32_next(t32, np.inf)
  for i, (fcs, novel) in enumerate([(t32, t32 < threshold), (below, True), (above, False), (float("nan"), False),
                                    (float("-inf"), True), (float("inf"), False), (-0.0, True)]):
    assert g.step(fcs, 0.25 + i, i, 0.5, threshold)[0] == int(novel)
  assert g.ref.size == 3 + int(t32 < threshold)


def test_gate_kernel_scripted_sequence_against_reference():
  """A few hundred steps: filling, duplicates, replacing and not replacing (u = 0 and the last double below 1 among them), the
  gate disabled, a machine that is not adapting."""
  rng = random.Random(11)
  g = _Gate(3)
  threshold = 10.0
  kinds = dict(append=0, dup=0, replace=0, no_replace=0, non_novel=0, off=0, idle=0)
  for step in range(300):
    fcs = rng.choice((9.0, 9.0, 9.0, 11.0, threshold, float("nan")))
    u = (0.0, U_LAST, rng.random(), rng.random() * 3.0 / (g.ref.offers + 1))[step % 4]
    idx = rng.randrange(6) if step < 150 else rng.randrange(1000)
    gate_enabled, adapting = rng.random() > 0.1, rng.random() > 0.1
    size, known = g.ref.size, idx in g.ref.indices[:g.ref.size]
    novel, slot, update = g.step(fcs, rng.uniform(0, 3), idx, u, threshold, gate_enabled, adapting)
    assert update == int(adapting and slot < 0)
    kinds["off"] += not gate_enabled; kinds["idle"] += not adapting
    kinds["non_novel"] += gate_enabled and not novel
    kinds["dup"] += bool(novel and known)
    kinds["append"] += bool(novel and not known and size < 3)
    kinds["replace"] += bool(novel and not known and size == 3 and slot >= 0)
    kinds["no_replace"] += bool(novel and not known and size == 3 and slot < 0)
  assert all(v > 0 for v in kinds.values()), kinds


def test_gate_kernel_capacity_one():
  g = _Gate(1)
  assert g.step(1.0, 0.5, 7, 0.3, 2.0) == (1, 0, 0)                 # appended
  assert g.step(1.0, 0.6, 7, 0.0, 2.0) == (1, -1, 1)                # duplicate: refused
  assert g.step(1.0, 0.7, 8, 0.0, 2.0) == (1, 0, 0)                 # r = 1: replaced; the index stays 7
  assert g.step(1.0, 0.8, 9, U_LAST, 2.0) == (1, -1, 1)             # r = offers = 4
  assert g.step(1.0, 0.9, 7, 0.0, 2.0) == (1, -1, 1)                # 7 is still the buffer's index: refused
  assert g.step(1.0, 1.0, 8, 0.0, 2.0) == (1, 0, 0)                 # 8 never entered the index set
  assert g.ref.indices == [7] and g.ref.state() == (1, 6, 3, 3)


def test_gate_kernel_offers_beyond_2_to_24():
  """The draw is taken in double and int64: with offers past 2^24 (where binary32 stops counting) every r is still exact."""
  g = _Gate(4)
  for i in range(4):
    g.step(0.0, 1.0, i, 0.5, 1.0)
  base = (1 << 24) + 3
  g.set_offers(base)
  for i, (u, slot) in enumerate([(0.0, 0), (3.5 / (base + 2), 3), (4.5 / (base + 3), -1), (U_LAST, -1),
                                 ((base + 3.5) / (base + 5), -1), (1.5 / (base + 6), 1)]):
    assert g.step(0.0, 2.0 + i, 100 + i, u, 1.0)[1] == slot, i
  assert g.ref.offers == base + 6
  big = (1 << 31) + 11                                             # and past int32
  g.set_offers(big)
  assert g.step(0.0, 9.0, 200, U_LAST, 1.0)[1] == -1 and g.step(0.0, 9.5, 201, 2.5 / (big + 2), 1.0)[1] == 2
  assert g.ref.offers == big + 2


# ---- as_reservoir_store ---------------------------------------------------------------------------------------------------
GUARD = 8           # a multiple of 4: dst_off = 0 puts slot 0 on a 16-byte boundary


@pytest.mark.parametrize("n", [3, 5, 1027, 5000, (1 << 20) + 1027])
@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (1, 0), (0, 1), (3, 2)])
def test_reservoir_store_between_guards(n, src_off, dst_off):
  """Every slot of a [capacity][n] buffer that starts `dst_off` floats past a 16-byte boundary, from sources `src_off` floats
  past one: the whole allocation — guards, other rows, the twin buffer — is compared byte for byte.  n = 2^20 + 1027 takes more
  than one trip of the grid-stride loop; rows of an odd n change alignment from slot to slot."""
  capacity = 3
  g = torch.Generator().manual_seed(n + 7 * src_off + dst_off)
  src = torch.rand(2, src_off + n + GUARD, generator=g).to(DEV)
  left, right = src[0, src_off:src_off + n], src[1, src_off:src_off + n]
  raw = torch.rand(2, dst_off + GUARD + capacity * n + GUARD, generator=g).to(DEV)
  lo = dst_off + GUARD
  bufs = [raw[i, lo:lo + capacity * n] for i in range(2)]
  slot = torch.zeros(1, dtype=torch.int32, device=DEV)
  expect = raw.clone()
  for s in (-1, capacity, 0, capacity - 1, 1, -5, 1 << 20):
    slot.fill_(s)
    nat.call("as_reservoir_store", nat.ptr(left), nat.ptr(right), n, nat.ptr(slot), capacity, nat.ptr(bufs[0]), nat.ptr(bufs[1]),
             nat.stream())
    if 0 <= s < capacity:
      expect[0, lo + s * n:lo + (s + 1) * n] = left
      expect[1, lo + s * n:lo + (s + 1) * n] = right
    assert torch.equal(raw, expect), "slot %d" % s
  assert torch.equal(src[0, src_off:src_off + n], left)


def test_device_reservoir_interface():
  r = DeviceReservoir(3, DEV)
  assert r.size() == 0 and len(r.buf) == 0
  left, right = torch.rand(1, 3, 4, 6, device=DEV), torch.rand(1, 3, 4, 6, device=DEV)
  r.allocate(left)
  one = lambda v, dt: torch.full((1,), v, dtype=dt, device=DEV)
  for i in range(2):
    r.gate(one(0.0, torch.float32), one(0.5 + i, torch.float32), one(40 + i, torch.int32), one(0.0, torch.float64), 1.0, True, True)
    r.store(left + i, right + i)
  assert r.size() == 2 and r.i == 2 and len(r.buf) == 2 and r.counters() == (2, 2, 2, 0)
  value, index, l, rr = r.buf[1]
  assert float(value) == 1.5 and index == 41 and torch.equal(l, left + 1) and torch.equal(rr, right + 1)
  assert r.average_value() == (0.5 + 1.5) / 2
  r.update_value(0, 0.75)
  assert r.average_value() == (0.75 + 1.5) / 2
  with pytest.raises(IndexError):
    r.buf[2]
  with pytest.raises(ValueError):
    r.allocate(torch.rand(1, 3, 4, 7, device=DEV))


# ---- gated clip + Adam -------------------------------------------------------------------------------------------------
N_OPT = 256 * 9 + 3          # several workgroups and a ragged end


class _Opt(object):
  def __init__(self, seed=5, lr_dev=False):
    g = torch.Generator().manual_seed(seed)
    self.p = torch.randn(N_OPT, generator=g).to(DEV)
    self.g = (torch.randn(N_OPT, generator=g) * 0.3).to(DEV)
    self.m = (torch.randn(N_OPT, generator=g) * 0.01).to(DEV)
    self.v = (torch.rand(N_OPT, generator=g) * 1e-3).to(DEV)
    self.step = torch.full((1,), 4.0, device=DEV)
    self.out, self.coef = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    self.ws = torch.empty(nat.load().as_sumsq_workspace(N_OPT), dtype=torch.float32, device=DEV)
    self.lr = 1e-3
    self.lr_dev = torch.full((1,), self.lr, device=DEV) if lr_dev else None

  def words(self):
    return [t.clone() for t in (self.p, self.m, self.v, self.step, self.out, self.coef)]

  def ungated(self):
    nat.call("as_sumsq_clip", nat.ptr(self.g), N_OPT, 1.0, nat.ptr(self.out), nat.ptr(self.coef), nat.ptr(self.step),
             nat.ptr(self.ws), nat.stream())
    if self.lr_dev is None:
      nat.call("as_adam_step", nat.ptr(self.p), nat.ptr(self.g), nat.ptr(self.m), nat.ptr(self.v), N_OPT, nat.ptr(self.coef),
               self.lr, 0.9, 0.999, 1e-8, 0, nat.ptr(self.step), nat.stream())
    else:
      nat.call("as_adam_step_lr", nat.ptr(self.p), nat.ptr(self.g), nat.ptr(self.m), nat.ptr(self.v), N_OPT, nat.ptr(self.coef),
               nat.ptr(self.lr_dev), 0.9, 0.999, 1e-8, 0, nat.ptr(self.step), nat.stream())

  def gated(self, gate):
    nat.call("as_sumsq_clip_gated", nat.ptr(self.g), N_OPT, 1.0, nat.ptr(self.out), nat.ptr(self.coef), nat.ptr(self.step),
             nat.ptr(self.ws), nat.ptr(gate), nat.stream())
    nat.call("as_adam_step_gated", nat.ptr(self.p), nat.ptr(self.g), nat.ptr(self.m), nat.ptr(self.v), N_OPT, nat.ptr(self.coef),
             self.lr, nat.ptr(self.lr_dev), 0.9, 0.999, 1e-8, 0, nat.ptr(self.step), nat.ptr(gate), nat.stream())


def _same(a, b):
  return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("lr_dev", [False, True])
def test_gated_optimizer_equals_ungated_and_holds_still(lr_dev):
  gate = torch.ones(1, dtype=torch.int32, device=DEV)
  a, b = _Opt(lr_dev=lr_dev), _Opt(lr_dev=lr_dev)
  for _ in range(2):
    a.ungated(); b.gated(gate)
    assert _same(a.words(), b.words())
  assert float(b.step) == 6.0 and float(b.coef) < 1.0               # the clip is active: coef rides into Adam
  gate.zero_()
  before = b.words()
  b.out.zero_(); b.coef.zero_()
  b.gated(gate)
  after = b.words()
  assert _same(before[:4], after[:4])                                # parameters, both moments, the step counter: untouched
  assert _same(before[4:], after[4:])                                # out and coef are written all the same
  gate.fill_(-3)                                                     # any non-zero flag is a go
  a.ungated(); b.gated(gate)
  assert _same(a.words(), b.words())


def test_gated_optimizer_under_graph_replay_with_the_flag_flipped():
  gate = torch.zeros(1, dtype=torch.int32, device=DEV)
  a, b = _Opt(), _Opt()
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    b.gated(gate)                                                    # warm-up with the gate shut: changes nothing
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    b.gated(gate)
  assert _same(a.words()[:4], b.words()[:4])
  for flag in (0, 1, 0, 0, 1, 1, 0):
    gate.fill_(flag)
    before = b.words()
    graph.replay()
    if flag:
      a.ungated()
      assert _same(a.words(), b.words()), flag
    else:
      assert _same(before[:4], b.words()[:4]), flag
  assert float(b.step) == 7.0


def test_fused_clip_adam_step_with_gate():
  """FusedClipAdam.step(gate=...) over a two-group arena: gate 1 is step(), gate 0 changes nothing, the host's step_count
  follows the device on refresh_step_count()."""
  def make():
    torch.manual_seed(3)
    mods = [torch.nn.Linear(37, 19).to(DEV), torch.nn.Linear(11, 5).to(DEV)]
    arena = FlatArena(mods)
    opt = FusedClipAdam(arena, 1e-3)
    return arena, opt
  (a1, o1), (a2, o2) = make(), make()
  gate = torch.ones(1, dtype=torch.int32, device=DEV)
  g = torch.Generator().manual_seed(9)
  for i in range(3):
    grads = (torch.randn(a1.numel, generator=g) * 0.5).to(DEV)
    a1.grads.copy_(grads); a2.grads.copy_(grads)
    gate.fill_(int(i != 1))
    before = [t.clone() for t in (a2.params, o2.exp_avg, o2.exp_avg_sq, o2.step_dev)]
    if i != 1:
      o1.step(clip=True)
    o2.step(clip=True, gate=gate)
    if i == 1:
      assert _same(before, [a2.params, o2.exp_avg, o2.exp_avg_sq, o2.step_dev])
    assert _same([a1.params, o1.exp_avg, o1.exp_avg_sq, o1.step_dev], [a2.params, o2.exp_avg, o2.exp_avg_sq, o2.step_dev])
  assert o2.step_count == 0 and o2.refresh_step_count() == 2 == o1.step_count
  with pytest.raises(ValueError):
    o2.step(clip=True, gate=torch.ones(1, device=DEV))
