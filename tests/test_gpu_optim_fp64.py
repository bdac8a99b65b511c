"""csrc/optim.hip through the C ABI: as_sumsq, as_sumsq_clip, as_clip_coef and as_adam_step against the float64 reference of
tests/adam_ref.py (held to torch.optim.Adam + clip_grad_norm_ on the CPU by tests/test_adam_ref_cpu.py), FusedClipAdam under
graph replay against eager stepping, and the two glue kernels as_relu_bwd and as_mirror_taps_ch0, which are exact.

Every Adam comparison is a one-step comparison from a given state, so each bound is a one-step bound (adam_ref's docstring
derives them): exp_avg and exp_avg_sq within 3 U of their term magnitudes, the update ``p_after - p_before`` within
``8 U |update| + ulp32(p_after) / 2`` of the float64 update computed from the stored moments.  The hyper-parameters of the
reference are the float32 values the ABI receives; their distance from torch's doubles is pinned on the CPU.  The gradient Adam
sees is the float32 product ``g * coef``, which is what clip_grad_norm_ stores as well.  Gradients are 0 or at least 1e-15 in
magnitude, so ``g g`` stays a normal number: how denormals are flushed is not pinned here.  The worst error / bound of every
group goes to conftest.parity_note.

What the numbers look like, and why.  exp_avg reaches 0.85 and exp_avg_sq 0.94 of their bounds: three roundings each, and among
half a million elements some have all three near their maximum.  The update reaches 0.99999 wherever |p| ~ 1: there the bound
is the half ulp of the final subtraction from p, which rounding to nearest attains; on the p = 0 quarter, where that term is
an ulp of the update itself, it stays below 0.5 (reported as update_at_p0_over_bound).  The exp_avg bound is what found the
one defect these tests exposed: with ``g * gs`` contracted into ``g * gs - m`` the kernel fed exp_avg the unrounded product and
exp_avg_sq the rounded one, and exp_avg stood at 1.03 (n = 313698) to 1.09 (n = 524545) of its bound whenever a clip
coefficient was passed; adam_kernel now rounds the product once (clipped_grad() in csrc/optim.hip)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from adaptive_stereo import _native as nat
from adaptive_stereo.adaptation import FlatArena, FusedClipAdam
import adam_ref as ar
from conftest import parity_note

DEV = "cuda:0"
LR, B1, B2, EPS = 5e-5, 0.9, 0.999, 1e-8
HP32 = ar.hyper(LR, B1, B2, EPS, True)
PATTERN = 0x7FC12345
GUARD = 64


def _gen(seed):
  return torch.Generator().manual_seed(seed)


def _log_uniform(n, lo, hi, g):
  """magnitudes 10^u, u uniform in [lo, hi], float32"""
  return torch.pow(10.0, torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()


def _signs(n, g):
  return (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()


class Slot(object):
  """n floats at a 16-byte aligned interior offset of a larger buffer (where FlatArena.group_bounds puts a group), the words
  around them a fixed bit pattern"""

  def __init__(self, values, off=20):
    n = values.numel()
    self.buf = torch.full((GUARD + off + n + GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    self.lo, self.hi = GUARD + off, GUARD + off + n
    self.view = self.buf.view(torch.float32)[self.lo:self.hi]
    self.view.copy_(values)
    assert self.view.data_ptr() % 16 == 0

  def get(self):
    torch.cuda.synchronize()
    b = self.buf.cpu()
    assert bool((b[:self.lo] == PATTERN).all()) and bool((b[self.hi:] == PATTERN).all()), "wrote outside the slice"
    return self.view.cpu()


def _ratio(err, bound):
  r = torch.where(err == 0, torch.zeros_like(err), err / bound)
  return float(r.max()) if r.numel() else 0.0


# =========================================================================================================== as_sumsq
def _workspace(n):
  """NaN in every word (and in every double made of two): a partial sum that is read without having been written shows"""
  return torch.full((nat.load().as_sumsq_workspace(n),), PATTERN, dtype=torch.int32, device=DEV).view(torch.float32)


def _sumsq(g):
  n = g.numel()
  gd = g.to(DEV)
  out = torch.full((1,), -1.0, device=DEV)
  ws = _workspace(n)
  nat.call("as_sumsq", nat.ptr(gd), n, nat.ptr(out), nat.ptr(ws), nat.stream())
  torch.cuda.synchronize()
  return out.cpu()


SUMSQ_N = [1, 255, 256, 257, 65535, 65536, 65537, 313698, 256 * 256 * 3 + 5]


@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq(n):
  """the kernel accumulates float64 in a fixed order and rounds once: within 1 ulp32 of the float64 sum plus n 2^-53 relative;
  uniform values, magnitudes from 1e-18 to 1e+15 in one vector, and exact zeros (a third of the elements, and all of them)"""
  worst = 0.0
  for kind in ("uniform", "span", "zeros"):
    g = _gen(n + 7)
    if kind == "uniform":
      x = (torch.rand(n, generator=g) * 2 - 1) * 1e-2
    elif kind == "span":
      x = _log_uniform(n, -18.0, 15.0, g) * _signs(n, g)
      x[torch.arange(n) % 3 == 1] = 0.0
    else:
      x = torch.zeros(n)
    got = _sumsq(x)
    again = _sumsq(x)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two runs differ"
    ref = float((x.double() ** 2).sum())
    if ref == 0.0:
      assert float(got) == 0.0
      continue
    bound = float(ar.ulp32(torch.tensor(ref))) + n * 2.0 ** -53 * ref
    worst = max(worst, abs(float(got.double()) - ref) / bound)
  parity_note("optim_sumsq_n%d" % n, worst_over_bound=worst)
  assert worst <= 1.0


def test_sumsq_refuses_an_unaligned_workspace():
  lib = nat.load()
  g = torch.ones(300, device=DEV)
  out = torch.full((1,), -1.0, device=DEV)
  ws = torch.empty(lib.as_sumsq_workspace(300) + 2, device=DEV)[1:]
  assert ws.data_ptr() % 8 == 4
  coef = torch.full((1,), -1.0, device=DEV)
  assert lib.as_sumsq(nat.ptr(g), 300, nat.ptr(out), nat.ptr(ws), nat.stream()) == -1
  assert "as_sumsq" in lib.as_last_error().decode()
  assert lib.as_sumsq_clip(nat.ptr(g), 300, 1.0, nat.ptr(out), nat.ptr(coef), None, nat.ptr(ws), nat.stream()) == -1
  torch.cuda.synchronize()
  assert float(out) == -1.0 and float(coef) == -1.0


# ============================================================================================= as_sumsq_clip, as_clip_coef
def _sumsq_clip(gd, max_norm, counter):
  n = gd.numel()
  out, coef = torch.full((1,), -1.0, device=DEV), torch.full((1,), -1.0, device=DEV)
  ws = _workspace(n)
  nat.call("as_sumsq_clip", nat.ptr(gd), n, max_norm, nat.ptr(out), nat.ptr(coef), nat.ptr(counter), nat.ptr(ws), nat.stream())
  torch.cuda.synchronize()
  return out.cpu(), coef.cpu()


def _ulps(a, b):
  return abs(int(a.view(torch.int32)) - int(b.view(torch.int32)))


@pytest.mark.parametrize("kind", ["below", "at", "above", "zero"])
def test_sumsq_clip_coefficient_and_counter(kind):
  """coef is bit-equal to min(max_norm / (sqrt(out) + 1e-6), 1) evaluated in float32 on the CPU from the stored ``out``; the
  counter moves by exactly 1 per call when passed and ``out`` / ``coef`` do not depend on it; as_clip_coef gives the same bits"""
  n, max_norm = 313698, 1.0
  g = torch.Generator().manual_seed(3)
  x = torch.rand(n, generator=g) * 2 - 1
  if kind == "below":
    x = x * 1e-4                       # norm ~ 0.03
  elif kind == "at":
    x = torch.zeros(n); x[0] = 1.0     # norm == max_norm exactly: coef = 1 / (1 + 1e-6) < 1
  elif kind == "zero":
    x = torch.zeros(n)
  gd = x.to(DEV)
  out0, coef0 = _sumsq_clip(gd, max_norm, None)
  counter = torch.tensor([41.0], device=DEV)
  out1, coef1 = _sumsq_clip(gd, max_norm, counter)
  assert float(counter) == 42.0
  out2, coef2 = _sumsq_clip(gd, max_norm, counter)
  assert float(counter) == 43.0
  for o, c in ((out1, coef1), (out2, coef2)):
    assert torch.equal(o.view(torch.int32), out0.view(torch.int32)) and torch.equal(c.view(torch.int32), coef0.view(torch.int32))
  plain = _sumsq(x)
  assert torch.equal(plain.view(torch.int32), out0.view(torch.int32)), "as_sumsq and as_sumsq_clip disagree"
  exp = ar.clip_coef32(out0, max_norm)
  d = _ulps(coef0.reshape(()), exp)
  outd = out0.to(DEV); coef3 = torch.full((1,), -1.0, device=DEV)
  nat.call("as_clip_coef", nat.ptr(outd), max_norm, nat.ptr(coef3), nat.stream())
  torch.cuda.synchronize()
  d3 = _ulps(coef3.cpu().reshape(()), exp)
  parity_note("optim_clip_coef_" + kind, ulps_sumsq_clip=d, ulps_clip_coef=d3, coef=float(coef0), sumsq=float(out0))
  assert d == 0 and d3 == 0
  if kind in ("below", "zero"):
    assert float(coef0) == 1.0
  else:
    assert float(coef0) < 1.0
  if kind == "at":
    assert float(out0) == 1.0
  if kind == "zero":                   # an all-zero gradient on a zero state: the update is 0, the parameters keep their bits
    p = torch.rand(n, generator=g)
    pd, m, v = p.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    coefd = coef0.to(DEV)
    nat.call("as_adam_step", nat.ptr(pd), nat.ptr(gd), nat.ptr(m), nat.ptr(v), n, nat.ptr(coefd), LR, B1, B2, EPS, 1, None,
             nat.stream())
    torch.cuda.synchronize()
    assert torch.equal(pd.cpu(), p) and float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0


# ========================================================================================================= as_adam_step
def _state(n, kind, seed, tiny=1e-15):
  """(p, g, m, v) float32 on the CPU.  Quarters of the vector: p = 0 (the update shows without the parameter's ulp), |p| ~ 1,
  |p| ~ 1e3, and again |p| ~ 1.  Every 16th element has g = 0 on a zero state (denominator eps, update 0).  kind 'first':
  m = v = 0; 'random': |m| ~ 1e-6 .. 1e-2 of either sign, v ~ 1e-8 .. 1e-2.  One gradient in a hundred has the
  magnitude ``tiny``, the others 1e-6 .. 1."""
  g = _gen(seed)
  idx = torch.arange(n)
  quarter = (idx * 4) // max(n, 1)
  p = (torch.rand(n, generator=g) * 2 - 1)
  p = torch.where(quarter == 0, torch.zeros(n), p)
  p = torch.where(quarter == 2, p * 1e3, p)
  grad = _log_uniform(n, -6.0, 0.0, g) * _signs(n, g)
  small = torch.rand(n, generator=g) < 0.01
  grad = torch.where(small, torch.full((n,), tiny) * _signs(n, g), grad)
  if kind == "first":
    m, v = torch.zeros(n), torch.zeros(n)
  else:
    m = _log_uniform(n, -6.0, -2.0, g) * _signs(n, g)
    v = _log_uniform(n, -8.0, -2.0, g)
  dead = idx % 16 == 15
  grad[dead] = 0.0; m[dead] = 0.0; v[dead] = 0.0
  return p, grad, m, v


def _adam(p, g, m, v, t, coef, counter):
  """one launch on slices at interior offsets -> (p, m, v) afterwards; ``counter`` True: the step comes from a device counter
  and the host argument is a wrong one on purpose"""
  ps, gs, ms, vs = Slot(p), Slot(g, off=4), Slot(m, off=36), Slot(v, off=0)
  cd = None if coef is None else torch.tensor([coef], dtype=torch.float32, device=DEV)
  sd = torch.tensor([float(t)], dtype=torch.float32, device=DEV) if counter else None
  assert sd is None or float(sd) == t
  nat.call("as_adam_step", nat.ptr(ps.view), nat.ptr(gs.view), nat.ptr(ms.view), nat.ptr(vs.view), p.numel(), nat.ptr(cd),
           LR, B1, B2, EPS, 7 if counter else t, nat.ptr(sd), nat.stream())
  out = ps.get(), ms.get(), vs.get()
  assert torch.equal(gs.get(), g), "the gradient was written"
  return out


def _judge_adam(p, g, m, v, t, coef, got):
  """-> worst error / bound of (m, v, update) for one step from (p, g, m, v)"""
  p1, m1, v1 = got
  gi = g if coef is None else g * torch.tensor(coef, dtype=torch.float32)        # float32 product, as clip_grad_norm_ stores it
  mr, vr, mt, vt = ar.moments(gi, m, v, HP32)
  rm = _ratio((m1.double() - mr).abs(), ar.K_STATE * ar.U * mt)
  rv = _ratio((v1.double() - vr).abs(), ar.K_STATE * ar.U * vt)
  upd = ar.update(m1, v1, t, HP32)
  got_upd = p1.double() - p.double()
  bound = ar.K_UPDATE * ar.U * upd.abs() + 0.5 * ar.ulp32(p1)
  ru = _ratio((got_upd - upd).abs(), bound)
  ru0 = _ratio((got_upd - upd).abs()[p == 0], bound[p == 0])          # where the parameter's own ulp does not dominate
  dead = (g == 0) & (m == 0) & (v == 0)
  assert torch.equal(p1[dead], p[dead]), "a zero gradient on a zero state moved a parameter"
  assert bool((v1 >= 0).all())
  return rm, rv, ru, ru0


STEPS = [1, 2, 3, 10, 1000, 100000, 2 ** 24 - 1]


@pytest.mark.parametrize("t", STEPS)
def test_adam_step_at_step_counts(t):
  """first-step and realistic states, with and without grad_scale; the host count and the device counter give identical bits"""
  n = 40000 + 257
  worst = [0.0, 0.0, 0.0, 0.0]
  for kind in ("first", "random"):
    for coef in (None, 0.37):
      p, g, m, v = _state(n, kind, seed=t % 1000 + (5 if kind == "first" else 9))
      host = _adam(p, g, m, v, t, coef, False)
      dev = _adam(p, g, m, v, t, coef, True)
      for a, b, name in zip(host, dev, "pmv"):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "host count and device counter differ in " + name
      worst = [max(a, b) for a, b in zip(worst, _judge_adam(p, g, m, v, t, coef, host))]
  parity_note("optim_adam_step%d" % t, m_over_bound=worst[0], v_over_bound=worst[1], update_over_bound=worst[2],
              update_at_p0_over_bound=worst[3])
  assert max(worst) <= 1.0


@pytest.mark.parametrize("n", [1, 255, 257, 313698, 2048 * 256 + 257])
def test_adam_step_sizes(n):
  """one element, around one workgroup, the production arena, and more than one pass of the grid-stride loop (2048 * 256)"""
  worst = [0.0, 0.0, 0.0, 0.0]
  for kind, coef, t, counter in (("first", 0.37, 1, True), ("random", None, 3, False), ("random", 0.81, 1000, True)):
    p, g, m, v = _state(n, kind, seed=n % 997)
    got = _adam(p, g, m, v, t, coef, counter)
    worst = [max(a, b) for a, b in zip(worst, _judge_adam(p, g, m, v, t, coef, got))]
  parity_note("optim_adam_n%d" % n, m_over_bound=worst[0], v_over_bound=worst[1], update_over_bound=worst[2],
              update_at_p0_over_bound=worst[3])
  assert max(worst) <= 1.0


def test_adam_trajectory_each_step_from_the_kernels_own_state():
  """five consecutive steps with the clip in front: the reference for step t + 1 starts from the kernel's state of step t"""
  n = 313698
  p, _, m, v = _state(n, "first", seed=77)
  worst = [0.0, 0.0, 0.0, 0.0]
  for t in range(1, 6):
    # (the norm is ~100 times these factors, so the clip scales by down to 3e-3: tiny gradients of 1e-12 keep g g normal)
    g = _state(n, "first", seed=100 + t, tiny=1e-12)[1] * [1e-3, 1.0, 1e-2, 3.0, 0.1][t - 1]
    out, coef = _sumsq_clip(g.to(DEV), 1.0, None)
    got = _adam(p, g, m, v, t, float(coef), True)
    worst = [max(a, b) for a, b in zip(worst, _judge_adam(p, g, m, v, t, float(coef), got))]
    p, m, v = got
  parity_note("optim_adam_trajectory", m_over_bound=worst[0], v_over_bound=worst[1], update_over_bound=worst[2],
              update_at_p0_over_bound=worst[3])
  assert max(worst) <= 1.0


# =================================================================================== FusedClipAdam: graph replay == eager
def _arena(seed):
  torch.manual_seed(seed)
  mods = [torch.nn.Linear(7, 5), torch.nn.Conv2d(3, 4, 3)]
  return FlatArena([m.to(DEV) for m in mods])


def _opt_state(opt):
  torch.cuda.synchronize()
  return [t.detach().cpu().clone() for t in (opt.arena.params, opt.exp_avg, opt.exp_avg_sq, opt.sumsq, opt.coef, opt.step_dev)]


def _same_bits(a, b, what):
  for x, y, name in zip(a, b, ("params", "exp_avg", "exp_avg_sq", "sumsq", "coef", "step_dev")):
    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "%s: %s differs" % (what, name)


def _grad_list(numel, steps):
  g = _gen(5)
  scales = [1e-3, 0.3, 2.0, 1e-2]
  return [((torch.rand(numel, generator=g) * 2 - 1) * scales[i % 4]).to(DEV) for i in range(steps)]


def test_fused_clip_adam_graph_replay_equals_eager_steps():
  """FusedClipAdam.step() captured once (one stream, no parallel branches) and replayed 20 times against 20 eager steps from the
  same start, the gradients rewritten between steps from a fixed list: every piece of state bit-equal, and step_dev == 20"""
  steps = 20
  eager_arena = _arena(1)
  assert all(s % 4 == 0 and e % 4 == 0 for s, e in eager_arena.group_bounds) and len(eager_arena.group_bounds) == 2
  grads = _grad_list(eager_arena.numel, steps)
  eager = FusedClipAdam(eager_arena, LR)
  for i in range(steps):
    eager_arena.grads.copy_(grads[i])
    eager.step()
  want = _opt_state(eager)
  assert float(want[5]) == steps and eager.step_count == steps
  assert 0.0 < float(want[4]) <= 1.0

  arena = _arena(1)
  opt = FusedClipAdam(arena, LR)
  arena.grads.copy_(grads[0])
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
    opt.step()
  torch.cuda.synchronize()
  assert float(opt.step_dev) == 0.0, "capturing ran the step"
  for i in range(steps):
    arena.grads.copy_(grads[i])
    graph.replay()
  _same_bits(_opt_state(opt), want, "graph replay")


@pytest.mark.parametrize("route", ["ride", "no_clip", "clip_group_1"])
def test_fused_clip_adam_device_counter_matches_the_host_count(route):
  """the device counter rides on the clip's finalize launch (clip of group 0), or moves with an add of its own (clip=False, a
  clip_group != 0): after k eager steps it is k, and each group's state is that of single as_adam_step launches given the host
  count k and the same inputs (bit-equal), so the counter was k when the step read it"""
  arena = _arena(2)
  grads = _grad_list(arena.numel, 3)
  opt = FusedClipAdam(arena, LR, clip_group=1 if route == "clip_group_1" else 0)
  p = arena.params.detach().clone(); m = torch.zeros_like(p); v = torch.zeros_like(p)
  clipped = {"ride": 0, "no_clip": None, "clip_group_1": 1}[route]
  for i in range(3):
    arena.grads.copy_(grads[i])
    opt.step(clip=(route != "no_clip"))
    torch.cuda.synchronize()
    assert float(opt.step_dev) == i + 1
    for gi, (s, e) in enumerate(arena.group_bounds):
      scale = None
      if gi == clipped:
        out, coef = _sumsq_clip(grads[i][s:e], 1.0, None)
        assert torch.equal(out, opt.sumsq.cpu()) and torch.equal(coef, opt.coef.cpu())
        scale = coef.to(DEV)
      nat.call("as_adam_step", nat.ptr(p[s:e]), nat.ptr(grads[i][s:e]), nat.ptr(m[s:e]), nat.ptr(v[s:e]), e - s, nat.ptr(scale),
               LR, B1, B2, EPS, i + 1, None, nat.stream())
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), arena.params.cpu()) and torch.equal(m.cpu(), opt.exp_avg.cpu()) and torch.equal(v.cpu(), opt.exp_avg_sq.cpu())


# ============================================================================================== as_relu_bwd, as_mirror_taps_ch0
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1027])
def test_relu_bwd_is_exact(n):
  """g_in = g_out where out > 0 else 0, with +0, -0, denormals of both signs and negatives in ``out``"""
  g = _gen(n)
  out = torch.rand(n, generator=g) * 2 - 1
  special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, -1.0, 1.0])
  k = torch.arange(n) % 11
  out = torch.where(k < 8, special[k.clamp_max(7)], out)
  go = torch.rand(n, generator=g) * 2 - 1
  od, gd = Slot(out), Slot(go, off=8)
  gin = Slot(torch.full((n,), float("nan")), off=12)
  nat.call("as_relu_bwd", nat.ptr(gd.view), nat.ptr(od.view), n, nat.ptr(gin.view), nat.stream())
  got = gin.get()
  exp = torch.where(out > 0, go, torch.zeros(n))
  assert torch.equal(got.view(torch.int32), exp.view(torch.int32))
  assert torch.equal(od.get().view(torch.int32), out.view(torch.int32)) and torch.equal(gd.get(), go)


def test_relu_bwd_refuses_a_misaligned_pointer():
  lib = nat.load()
  buf = torch.zeros(3, 64, device=DEV)
  for which in range(3):
    ptrs = [nat.ptr(buf[i][1:] if i == which else buf[i]) for i in range(3)]
    assert lib.as_relu_bwd(ptrs[0], ptrs[1], 8, ptrs[2], nat.stream()) == -1
    assert "as_relu_bwd" in lib.as_last_error().decode()


@pytest.mark.parametrize("Cin", [1, 4, 32])
@pytest.mark.parametrize("which", ["by_tap", "by_channel", "both"])
def test_mirror_taps_ch0_is_exact(Cin, which):
  """by_tap[t][c] = by_channel[c][t] = w[c][0][8 - t] for a [32][Cin][3][3] weight; each layout alone and both together"""
  w = torch.rand(32, Cin, 3, 3, generator=_gen(Cin))
  wd = w.to(DEV)
  nan = torch.full((288,), float("nan"))
  by_tap = Slot(nan) if which in ("by_tap", "both") else None
  by_channel = Slot(nan, off=8) if which in ("by_channel", "both") else None
  nat.call("as_mirror_taps_ch0", nat.ptr(wd), Cin, nat.ptr(by_tap.view) if by_tap else None,
           nat.ptr(by_channel.view) if by_channel else None, nat.stream())
  mirrored = w[:, 0].reshape(32, 9).flip(1)            # [c][t] = w[c][0][8 - t]
  if by_tap:
    assert torch.equal(by_tap.get().view(9, 32), mirrored.t().contiguous())
  if by_channel:
    assert torch.equal(by_channel.get().view(32, 9), mirrored)
