"""csrc/proxy_loss.hip on the device, between guard elements.

  as_proxy_term_fwd   counts exact; loss and denominator bit for bit as_khamis_fwd's out2 on where(code == 0, disp, 0), the sum the
                      float32 whose quotient by the count is that loss; epe and bad within 1 float32 ulp of the reference's
                      math.fsum (one rounding of an fp64 sum whose own error, n * 2^-53, is far below it: the bound
                      test_gpu_supervised.py uses for as_khamis2_fwd: |disp - pred| is exact arithmetic per pixel).  The sum against
                      the reference's: within count * VALUE_ULPS per-pixel ulps.  The device's value chain is khamis_fwd_kernel's:
                      fma(d, d, 4), the hardware's square root, fma(s, 0.5, -1), not the five separately rounded operations of
                      numpy (seen two ulps of the value apart at d = 2.9999998), so the per-pixel values agree only that far
  as_proxy_term_bwd   bit for bit as_khamis_bwd on the same labels, exactly +0.0 off the label set, and BOTH bit for bit the
                      uncontracted float32 restatement proxy_loss_ref.backward (IEEE multiply, add, square root and division in
                      the written order): the pin of as_khamis_bwd's bits
Sizes: 1, 63 .. 65 (a wave), 255 .. 257 (a workgroup), 4099 (several workgroups, n % 4 = 3) and 131072 + 1027, the first past
512 x 256 at which the stride loop takes a second trip.  Bases: pred / disp / g_pred one float off 16 bytes, code one and three
bytes off.  Then the planted edges of tests/test_proxy_loss_ref_cpu.py, NaN containment, outputs overwritten by a second call, a
captured graph replayed twice on a second input, and every refusal with nothing written."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from adaptive_stereo import _native as nat
from adaptive_stereo import hip_ops
import proxy_loss_ref as pl

DEV = "cuda:0"
F = np.float32
GUARD = 64                      # elements: 256 bytes of fp32, 64 of uint8 — an offset of 0 keeps the view 16-byte aligned
SENTINEL, SENTINEL_U8 = -7777.0, 0xA5
SIZES = (1, 63, 64, 65, 255, 256, 257, 4099, 131072 + 1027)
OFFSETS = ((0, 0), (1, 1), (0, 3), (1, 0))          # (floats off for pred / disp / g_pred, bytes off for code)


class Placed(object):
  """n elements at ``off`` elements past a 16-byte aligned address, sentinels before and behind"""

  def __init__(self, n, off=0, dtype=torch.float32, values=None):
    fill = SENTINEL_U8 if dtype == torch.uint8 else SENTINEL
    self.raw = torch.full((2 * GUARD + off + n,), fill, dtype=dtype, device=DEV)
    self.lo, self.hi, self.fill = GUARD + off, GUARD + off + n, fill
    self.view = self.raw[self.lo:self.hi]
    assert self.raw.data_ptr() % 16 == 0
    if values is not None:
      self.view.copy_(torch.as_tensor(values).to(dtype))

  def untouched(self):
    return bool((self.view == self.fill).all())

  def result(self):
    assert bool((self.raw[:self.lo] == self.fill).all()) and bool((self.raw[self.hi:] == self.fill).all()), "guard overwritten"
    return self.view.cpu().numpy()


def _place(pred, disp, code, off_f=0, off_c=0):
  n = len(pred)
  return (Placed(n, off_f, values=pred), Placed(n, off_f, values=disp), Placed(n, off_c, torch.uint8, code))


def _workspace(n):
  return torch.empty(nat.load().as_proxy_term_workspace(n), dtype=torch.float32, device=DEV)


def _fwd(placed, bad_px=3.0):
  n = placed[0].view.numel()
  out6 = Placed(6)
  nat.call("as_proxy_term_fwd", nat.ptr(placed[0].view), nat.ptr(placed[1].view), nat.ptr(placed[2].view), n, float(bad_px),
           nat.ptr(out6.view), nat.ptr(_workspace(n)), nat.stream())
  return out6


def _bwd(placed, out6, g_loss, off_f=0):
  n = placed[0].view.numel()
  g = torch.full((1,), float(g_loss), dtype=torch.float32, device=DEV)
  g_pred = Placed(n, off_f)
  nat.call("as_proxy_term_bwd", nat.ptr(placed[0].view), nat.ptr(placed[1].view), nat.ptr(placed[2].view), nat.ptr(g), nat.ptr(out6.view),
           n, nat.ptr(g_pred.view), nat.stream())
  return g_pred.result()


def _khamis(pred_dev, labels_dev, g_loss):
  """as_khamis_fwd / as_khamis_bwd on the materialised labels -> (out2, g_pred) as numpy"""
  n = pred_dev.numel()
  out2 = torch.empty(2, dtype=torch.float32, device=DEV)
  ws = torch.empty(nat.load().as_khamis_workspace(n), dtype=torch.float32, device=DEV)
  nat.call("as_khamis_fwd", nat.ptr(pred_dev), nat.ptr(labels_dev), n, nat.ptr(out2), nat.ptr(ws), nat.stream())
  g = torch.full((1,), float(g_loss), dtype=torch.float32, device=DEV)
  g_pred = torch.empty(n, dtype=torch.float32, device=DEV)
  nat.call("as_khamis_bwd", nat.ptr(pred_dev), nat.ptr(labels_dev), nat.ptr(g), nat.ptr(out2), n, nat.ptr(g_pred), nat.stream())
  return out2.cpu().numpy(), g_pred.cpu().numpy()


def _bits(a):
  return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _ulp32(x):
  return float(np.spacing(F(abs(x))))


def _within_one_ulp(got, ref64, what):
  err, ulp = abs(float(got) - ref64), (_ulp32(ref64) if ref64 != 0 else 0.0)
  print("%s: %r against %r (%.3f ulp)" % (what, float(got), ref64, err / ulp if ulp else 0.0))
  assert err <= ulp, what


# In ulps of s / 2 = v + 1 the device's chain is within 0.25 (fma(d, d, 4) through the root) + 1 (the hardware's root) + 0.5 (the
# last fma) = 1.75 of the exact value and numpy's within 0.5 (d * d and + 4 through the root) + 0.5 (the root) + 0.5 (the
# subtraction) = 1.5: up to 3.25 between them at worst.  The bound was set at 2 and stays there, below the worst case: the
# inputs are seeded and fixed, and a pixel beyond 2 would be worth a look.
VALUE_ULPS = 2


def _value_tolerance(v_max):
  return VALUE_ULPS * float(np.spacing(F(v_max + 1.0)))


def _reference_sums(pred, disp, code, bad_px):
  m, v, e = pl.pixel_terms(pred, disp, code)
  count = int(m.sum())
  nv = max(count, 1)
  return (count, (math.fsum(v[m].astype(np.float64).tolist()), float(v[m].max()) if count else 0.0),
          math.fsum(e[m].astype(np.float64).tolist()) / nv, float((e > F(bad_px))[m].sum()) / nv, m)


@pytest.fixture(scope="module")
def cases():
  """(pred, disp, code) per size, and its reference sums: computed once, never written to"""
  made = {}
  for n in SIZES:
    pred, disp, code = pl.planted_case(n, seed=n)
    if n == 1:
      disp[0], code[0] = F(7.5), 0
    made[n] = (pred, disp, code, _reference_sums(pred, disp, code, 3.0))
  return made


# ================================================================================================================ both entry points
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_misaligned_bases(n, cases):
  pred, disp, code, (count, (S, v_max), epe, bad, m) = cases[n]
  assert n == 1 or 0 < count < n
  g_loss = 0.75
  for off_f, off_c in OFFSETS:
    what = "n=%d off=%d/%d" % (n, off_f, off_c)
    placed = _place(pred, disp, code, off_f, off_c)
    assert placed[0].view.data_ptr() % 16 == 4 * off_f and placed[2].view.data_ptr() % 4 == off_c
    out6_dev = _fwd(placed)
    out6 = out6_dev.result()
    labels = torch.where(placed[2].view == 0, placed[1].view, torch.zeros((), device=DEV)).contiguous()
    out2, g_khamis = _khamis(placed[0].view.contiguous(), labels, g_loss)
    assert out6[5] == count and out6[1] == max(count, 1), what                        # exact
    assert np.array_equal(_bits(out6[:2]), _bits(out2)), (what, out6, out2)           # bit for bit as_khamis_fwd
    assert _bits(F(out6[2]) / F(out6[1])) == _bits(out6[0]), what                     # ... and so is the sum it divided
    print("%s sum: %r against %r" % (what, float(out6[2]), S))
    assert abs(float(out6[2]) - S) <= count * _value_tolerance(v_max) + _ulp32(S), what
    _within_one_ulp(out6[3], epe, what + " epe")
    _within_one_ulp(out6[4], bad, what + " bad")
    g_pred = _bwd(placed, out6_dev, g_loss, off_f)
    assert np.array_equal(_bits(g_pred), _bits(g_khamis)), what                       # bit for bit as_khamis_bwd
    assert np.all(_bits(g_pred[~m]) == 0), what                                       # exactly +0.0 off the label set
    ref = pl.backward(pred, disp, code, g_loss, out6)
    assert np.array_equal(_bits(g_khamis), _bits(ref)), what                          # as_khamis_bwd: the uncontracted restatement's bits
    assert np.array_equal(_bits(g_pred), _bits(ref)), what
    for p in placed:
      p.result()                                                                      # inputs and their guards as they were


def test_deterministic(cases):
  pred, disp, code, _ = cases[131072 + 1027]
  placed = _place(pred, disp, code)
  a, b = _fwd(placed).result(), _fwd(placed).result()
  assert np.array_equal(_bits(a), _bits(b))


# ================================================================================================================ planted edges
EDGES = [
  ("no label", [1.0, 2.0, 3.0, 4.0], [0.0, -1.0, 5.0, np.nan], [0, 0, 3, 0], 3.0),
  ("one label", [9.0, 5.0, 9.0, 9.0, 9.0], [9.0, 8.0, 9.0, 9.0, 9.0], [1, 0, 2, 6, 7], 2.5),
  ("two labels, NaN under a code", [1.0, np.nan, 4.0], [1.0, 5.0, 8.0], [0, 5, 0], 3.0),
  ("unusable disparities", [2.0] * 4, [np.nan, -0.0, 0.0, -3.0], [0, 0, 0, 0], 3.0),
  ("infinity is a label", [2.0] * 5, [np.nan, -0.0, 0.0, -3.0, np.inf], [0] * 5, 3.0),
  ("codes 1..7", [0.0] * 7, [5.0] * 7, [1, 2, 3, 4, 5, 6, 7], 3.0),
  ("codes 128 and 255", [0.0] * 2, [5.0] * 2, [255, 128], 3.0),
  ("bad_px below", [0.0], [np.nextafter(F(3.0), F(0))], [0], 3.0),
  ("bad_px exactly", [0.0], [3.0], [0], 3.0),
  ("bad_px above", [0.0], [np.nextafter(F(3.0), F(10))], [0], 3.0),
  ("bad_px 0", [1.0, 2.0], [2.0, 2.0], [0, 0], 0.0),
]


@pytest.mark.parametrize("name,pred,disp,code,bad_px", EDGES, ids=[e[0] for e in EDGES])
def test_planted_edges(name, pred, disp, code, bad_px):
  pred, disp, code = np.array(pred, F), np.array(disp, F), np.array(code, np.uint8)
  placed = _place(pred, disp, code)
  out6_dev = _fwd(placed, bad_px)
  out6, ref = out6_dev.result(), pl.forward(pred, disp, code, bad_px)
  # at most five labels: the fp64 sums are exact in any order, so denominator, epe, bad and count carry the reference's roundings;
  # loss and sum are as_khamis_fwd's bits, and the reference's within the two chains' difference per pixel
  print(name, out6, ref)
  assert np.array_equal(_bits(out6[[1, 3, 4, 5]]), _bits(ref[[1, 3, 4, 5]])), (out6, ref)
  labels = torch.from_numpy(pl.materialised_labels(disp, code)).to(DEV)
  out2, _ = _khamis(placed[0].view, labels, 1.0)
  assert np.array_equal(_bits(out6[:2]), _bits(out2)) and _bits(F(out6[2]) / F(out6[1])) == _bits(out6[0]), (out6, out2)
  m = pl.labelled(disp, code)
  if np.isinf(ref[0]):
    assert out6[0] == ref[0] and out6[2] == ref[2]
  else:
    tol = _value_tolerance(float(pl.pixel_terms(pred, disp, code)[1].max())) * max(int(m.sum()), 1)
    assert abs(float(out6[2]) - float(ref[2])) <= tol and abs(float(out6[0]) - float(ref[0])) <= tol, (out6, ref, tol)
  g_pred = _bwd(placed, out6_dev, 1.0)
  assert np.all(_bits(g_pred[~m]) == 0)
  if name == "no label":
    assert out6.tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
  if name == "bad_px exactly":
    assert out6[4] == 0.0 and out6[3] == 3.0
  if name == "bad_px above":
    assert out6[4] == 1.0


def test_nan_under_a_non_zero_code_changes_nothing(cases):
  pred, disp, code, (_, _, _, _, m) = cases[4099]
  clean = _place(pred, disp, code)
  out_clean = _fwd(clean)
  poisoned_pred = np.where(~m, F(np.nan), pred).astype(F)              # NaN wherever there is no label (non-zero code or bad disp)
  assert np.isnan(poisoned_pred).sum() > 100 and (code[np.isnan(poisoned_pred)] != 0).any()
  dirty = _place(poisoned_pred, disp, code)
  out_dirty = _fwd(dirty)
  assert np.array_equal(_bits(out_clean.result()), _bits(out_dirty.result()))
  assert np.array_equal(_bits(_bwd(clean, out_clean, 0.5)), _bits(_bwd(dirty, out_dirty, 0.5)))


def test_outputs_are_overwritten_by_a_second_call(cases):
  pred, disp, code, _ = cases[4099]
  n = len(pred)
  first, second = _place(pred, disp, code), _place(pred, disp, np.full(n, 6, np.uint8))       # then: not one label
  out6, ws = Placed(6), _workspace(n)
  g, g_pred = torch.ones(1, device=DEV), Placed(n)
  for placed in (first, second):
    nat.call("as_proxy_term_fwd", nat.ptr(placed[0].view), nat.ptr(placed[1].view), nat.ptr(placed[2].view), n, 3.0, nat.ptr(out6.view),
             nat.ptr(ws), nat.stream())
    nat.call("as_proxy_term_bwd", nat.ptr(placed[0].view), nat.ptr(placed[1].view), nat.ptr(placed[2].view), nat.ptr(g),
             nat.ptr(out6.view), n, nat.ptr(g_pred.view), nat.stream())
  assert out6.result().tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
  assert np.all(_bits(g_pred.result()) == 0)


# ================================================================================================================ the autograd node, captured
def test_node_and_captured_replay_on_a_second_input(cases):
  n = 4099
  pred_a, disp_a, code_a, _ = cases[n]
  pred_b, disp_b, code_b = pl.planted_case(n, seed=99)
  dev = lambda a: torch.from_numpy(a).to(DEV)

  def eager(pred, disp, code):
    p = dev(pred).requires_grad_(True)
    loss, out6 = hip_ops.ProxyTermFn.apply(p, dev(disp), dev(code), 3.0)
    assert not out6.requires_grad and loss.requires_grad
    (2.0 * loss).backward()
    return loss.detach().cpu().numpy(), out6.cpu().numpy(), p.grad.cpu().numpy()

  want_a, want_b = eager(pred_a, disp_a, code_a), eager(pred_b, disp_b, code_b)
  assert want_a[1][5] != want_b[1][5]
  assert np.array_equal(_bits(want_a[0]), _bits(want_a[1][0]))
  placed = _place(pred_a, disp_a, code_a)
  out6_dev = _fwd(placed)
  assert np.array_equal(_bits(want_a[1]), _bits(out6_dev.result())) and np.array_equal(_bits(want_a[2]), _bits(_bwd(placed, out6_dev, 2.0)))

  sp, sd, sc = dev(pred_a).requires_grad_(True), dev(disp_a), dev(code_a)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
    loss, out6 = hip_ops.ProxyTermFn.apply(sp, sd, sc, 3.0)
    grad, = torch.autograd.grad(2.0 * loss, sp)
  with torch.no_grad():
    sp.copy_(dev(pred_b)); sd.copy_(dev(disp_b)); sc.copy_(dev(code_b))
  for _ in range(2):
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(loss.detach().cpu().numpy()), _bits(want_b[0]))
    assert np.array_equal(_bits(out6.cpu().numpy()), _bits(want_b[1]))
    assert np.array_equal(_bits(grad.cpu().numpy()), _bits(want_b[2]))


def test_node_refuses_what_it_cannot_read_in_place():
  p = torch.zeros(2, 1, 4, 6, device=DEV)
  with pytest.raises(RuntimeError, match="contiguous"):
    hip_ops.ProxyTermFn.apply(p, torch.zeros(2, 1, 4, 12, device=DEV)[..., ::2], torch.zeros(2, 1, 4, 6, dtype=torch.uint8, device=DEV), 3.0)
  with pytest.raises(RuntimeError, match="uint8"):
    hip_ops.ProxyTermFn.apply(p, torch.zeros_like(p), torch.zeros_like(p), 3.0)
  with pytest.raises(RuntimeError, match="shape"):
    hip_ops.ProxyTermFn.apply(p, torch.zeros(2, 1, 4, 5, device=DEV), torch.zeros(2, 1, 4, 6, dtype=torch.uint8, device=DEV), 3.0)


# ================================================================================================================ refusals
def test_every_refusal_leaves_the_outputs_untouched(cases):
  pred, disp, code, _ = cases[257]
  n = len(pred)
  lib = nat.load()
  P, D, C = _place(pred, disp, code)
  out6, g_pred, ws = Placed(6), Placed(n), Placed(lib.as_proxy_term_workspace(n))
  good6 = _fwd((P, D, C))
  g = torch.ones(1, device=DEV)
  ptr, st = nat.ptr, nat.stream()
  off1 = lambda t: nat.c_vp(t.data_ptr() + 4)
  fwd = [
    (None, ptr(D.view), ptr(C.view), n, 3.0, ptr(out6.view), ptr(ws.view), st),
    (ptr(P.view), None, ptr(C.view), n, 3.0, ptr(out6.view), ptr(ws.view), st),
    (ptr(P.view), ptr(D.view), None, n, 3.0, ptr(out6.view), ptr(ws.view), st),
    (ptr(P.view), ptr(D.view), ptr(C.view), n, 3.0, None, ptr(ws.view), st),
    (ptr(P.view), ptr(D.view), ptr(C.view), n, 3.0, ptr(out6.view), None, st),
    (ptr(P.view), ptr(D.view), ptr(C.view), 0, 3.0, ptr(out6.view), ptr(ws.view), st),
    (ptr(P.view), ptr(D.view), ptr(C.view), -n, 3.0, ptr(out6.view), ptr(ws.view), st),
    (ptr(P.view), ptr(D.view), ptr(C.view), n, 3.0, ptr(out6.view), off1(ws.view), st),                 # workspace off 8 bytes
    (ptr(P.view), ptr(D.view), ptr(C.view), n, -0.5, ptr(out6.view), ptr(ws.view), st),
    (ptr(P.view), ptr(D.view), ptr(C.view), n, float("nan"), ptr(out6.view), ptr(ws.view), st),
    (ptr(P.view), ptr(D.view), ptr(C.view), n, float("inf"), ptr(out6.view), ptr(ws.view), st),
  ]
  bwd = [
    (None, ptr(D.view), ptr(C.view), ptr(g), ptr(good6.view), n, ptr(g_pred.view), st),
    (ptr(P.view), None, ptr(C.view), ptr(g), ptr(good6.view), n, ptr(g_pred.view), st),
    (ptr(P.view), ptr(D.view), None, ptr(g), ptr(good6.view), n, ptr(g_pred.view), st),
    (ptr(P.view), ptr(D.view), ptr(C.view), None, ptr(good6.view), n, ptr(g_pred.view), st),
    (ptr(P.view), ptr(D.view), ptr(C.view), ptr(g), None, n, ptr(g_pred.view), st),
    (ptr(P.view), ptr(D.view), ptr(C.view), ptr(g), ptr(good6.view), n, None, st),
    (ptr(P.view), ptr(D.view), ptr(C.view), ptr(g), ptr(good6.view), 0, ptr(g_pred.view), st),
    (ptr(P.view), ptr(D.view), ptr(C.view), ptr(g), ptr(good6.view), n, ptr(P.view), st),               # in place over pred
    (ptr(P.view), ptr(D.view), ptr(C.view), ptr(g), ptr(good6.view), n, off1(D.view), st),              # overlapping disp
  ]
  for name, rows in (("as_proxy_term_fwd", fwd), ("as_proxy_term_bwd", bwd)):
    for i, args in enumerate(rows):
      assert getattr(lib, name)(*args) == -1, (name, i)
      assert name.encode() in lib.as_last_error(), (name, i, lib.as_last_error())
  torch.cuda.synchronize()
  assert out6.untouched() and g_pred.untouched() and ws.untouched()
  out6.result(); g_pred.result(); ws.result()
  assert np.array_equal(P.result(), pred) and np.array_equal(_bits(D.result()), _bits(disp)) and np.array_equal(C.result(), code)
