"""AdaptationLoop(captured=True) against the host-side loop from the same state, bit for bit: parameters, both Adam moments,
the step count, every BatchNorm buffer, the reservoir's slots and values, the state machine's events, and per step the loss,
the FCS, its EMA and the flags.

The stream: 40 steps of one pair, 64x96, k = 3, maxdisp 64, a reservoir of two slots validated every 4 steps.  With these
synthetic weights the FCS is a property of the networks more than of the pair: it starts near 3 and climbs past 11 within some
twenty updates at lr 1e-3 (more slowly with a replay term).  THRESHOLD sits in that climb, so the first phase is novel (appends, refused duplicates of repeated
batch indices, replacements and non-replacements steered by the uniforms, skipped updates) and the rest is not.  Steps 24-31
are the same kind of pair at 0.15 of the brightness: train-mode BatchNorm hides that from the step, but the first layer's running
statistics follow it, the eval-mode validation of the (bright) reservoir pairs gets worse and the machine goes to DONE (with the
replay term it goes there earlier, on a validation that did not improve, and a dip of the FCS restarts it by itself).  No
pair was found that these adapted networks score below the threshold (in eval mode every family scores above 14), so the domain
change that restarts the machine is played on the score itself: before step 32 the FCS EMA of either loop is set to PUSH_VALUE,
which makes steps 32 and 33 novel.  That the HOST loop's own record shows every kind of step is asserted from that record
(_coverage).  random.randint of the host loop and random.random of the captured loop are
both patched onto one list of uniforms indexed by the step, which makes the two reservoirs draw alike."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from adapt_gate_ref import randint_from_uniform
from adaptive_stereo import control
from adaptive_stereo.adaptation import OnlineAdapter
from adaptive_stereo.control import AdaptationLoop, State
from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
from adaptive_stereo.utils import stereo_reservoir
from adaptive_stereo.utils import synthetic as syn

DEV = "cuda:0"
K, MAXDISP, H, W = 3, 64, 64, 96
STEPS = 40
CAPACITY, VALIDATE_HZ, RETRIES = 2, 4, 1
EMA_WEIGHT = 0.3            # a short memory: the smoothed FCS follows the raw one within two steps
LR = 1e-3
# the replay term slows the climb of the FCS (VS+ER reaches 6 where VS reaches 10), so the threshold that splits the run differs
THRESHOLD = {"VS": 7.8, "VS+ER": 5.5, "ER": 7.8, "NONSTOP": 7.8}
# pair per step: "n" = two unrelated images, "f" = a shifted pair, "d" = a shifted pair at 0.15 of the brightness
FAMILIES = "nnnnnnnn" "ffffffff" "ffffffff" "dddddddd" "ffffffff"
PUSH_STEP, PUSH_VALUE = 32, -100.0
# batch indices: repeats while the gate is open make refused duplicates; fresh ones meet a full buffer
BATCH_IDX = [0, 1, 0, 2, 3, 1, 4, 5] + list(range(8, 32)) + [0, 50, 51, 52] + list(range(60, 64))
# uniforms per step: 0.0 always replaces (r = 1), 0.999 never does (r = offers) once offers > capacity
UNIFORMS = [0.0, 0.999, 0.0, 0.0, 0.999, 0.0, 0.999, 0.0] * 5


def build():
  fnet, snet = FeatureExtractorNetwork(K), StereoNet(K, 1, 0, maxdisp=MAXDISP)
  fnet.load_state_dict(syn.synthetic_state_dict(fnet.state_dict(), seed=123))
  snet.load_state_dict(syn.synthetic_state_dict(snet.state_dict(), seed=123, logit_gain=5.0))
  return fnet.to(DEV), snet.to(DEV)


def familiar_pair(seed):
  left, right = syn.stereo_pair(1, H, W, seed=seed, disparities=(3.0 + seed % 5,))
  return left.to(DEV), right.to(DEV)


def novel_pair(seed):
  """Two unrelated images: nothing in the right image matches the left one."""
  left, _ = syn.stereo_pair(1, H, W, seed=1000 + seed)
  right, _ = syn.stereo_pair(1, H, W, seed=2000 + seed)
  return left.to(DEV), right.to(DEV)


def dark_pair(seed):
  left, right = familiar_pair(seed)
  return left * 0.15, right * 0.15


@pytest.fixture(scope="module")
def stream():
  make = {"n": novel_pair, "f": familiar_pair, "d": dark_pair}
  pairs = [make[f](i) for i, f in enumerate(FAMILIES)]
  g = torch.Generator().manual_seed(77)
  replay = []
  for i in range(3):
    l, r = familiar_pair(500 + i)
    gt = (torch.rand(1, 1, H, W, generator=g) * 20 + 1).to(DEV)
    replay.append((l, r, gt))
  return pairs, replay


def _loop(mode, captured, retries=RETRIES):
  fnet, snet = build()
  adapter = OnlineAdapter(fnet, snet, H, W, lr=LR, fcs_ema_weight=EMA_WEIGHT)
  return AdaptationLoop(adapter, mode=mode, ovs_buffer_size=CAPACITY, ovs_validate_hz=VALIDATE_HZ, val_improve_retries=retries,
                        ood_threshold=THRESHOLD[mode], er_loss_weight=0.05, captured=captured)


def _run(mode, captured, stream, monkeypatch):
  """-> (loop, per-step record, the state machine's events: ("validated", step, OVS loss, state after) and ("restart", step))."""
  pairs, replay = stream
  loop = _loop(mode, captured)
  sm, events = loop.state_machine, []
  transition, restart = sm.transition, sm.restart

  def logged_transition(retries):
    state = transition(retries)
    events.append(("validated", loop.step, float(sm.ovs.average_value()), state))
    return state

  def logged_restart():
    events.append(("restart", loop.step))
    restart()
  sm.transition, sm.restart = logged_transition, logged_restart
  monkeypatch.setattr(stereo_reservoir.random, "randint", lambda a, b: randint_from_uniform(UNIFORMS[loop.step], b))
  monkeypatch.setattr(control.random, "random", lambda: UNIFORMS[loop.step])
  record = []
  for i in range(STEPS):
    state_before = sm.state()
    if i == PUSH_STEP and mode != "NONSTOP":
      loop.adapter.fcs_smoothed.fill_(PUSH_VALUE)
    rep = replay[i % len(replay)] if mode in ("ER", "VS+ER") else None
    res = loop.process(pairs[i][0].clone(), pairs[i][1].clone(), BATCH_IDX[i], replay=rep)
    record.append(dict(state_before=state_before, state=res["state"], loss=float(res["loss"]), fcs=float(res["fcs"]),
                       fcs_smoothed=float(res["fcs_smoothed"]), updated=int(res["updated"]), added=int(res["added_to_ovs"]),
                       replay_loss=None if res.get("replay_loss") is None else float(res["replay_loss"])))
  loop.sync()
  torch.cuda.synchronize()
  return loop, record, events


def _final_words(loop):
  a = loop.adapter
  words = {"params": a.arena.params, "exp_avg": a.optimizer.exp_avg, "exp_avg_sq": a.optimizer.exp_avg_sq,
           "step_dev": a.optimizer.step_dev, "fcs_smoothed": a.fcs_smoothed}
  for tag, net in (("stereo_net", a.stereo_net), ("feature_net", a.feature_net)):
    for name, b in net.named_buffers():
      words["%s.%s" % (tag, name)] = b
  return {k: v.detach().clone() for k, v in words.items()}


def _assert_same_words(a, b):
  assert a.keys() == b.keys()
  for key in a:
    assert a[key].dtype == b[key].dtype and torch.equal(a[key], b[key]), key


def _coverage(record, events, loop):
  """What the HOST loop's record shows, by kind of step."""
  seen = dict(non_novel=0, append=0, duplicate=0, replace=0, no_replace=0, skipped_update=0, done=0, restart=0)
  ovs, size, known = loop.state_machine.ovs, 0, set()
  for i, r in enumerate(record):
    novel = r["fcs_smoothed"] < loop.ood_threshold
    seen["non_novel"] += not novel
    if novel:
      dup = BATCH_IDX[i] in known
      seen["duplicate"] += dup
      if not dup and size < CAPACITY:
        assert r["added"]
        seen["append"] += 1; size += 1; known.add(BATCH_IDX[i])
      elif not dup:
        seen["replace"] += r["added"]; seen["no_replace"] += not r["added"]
    seen["skipped_update"] += bool(r["added"] and r["state_before"] == State.IN_PROGRESS)
  assert size == ovs.size() and known == ovs.indices
  seen["done"] = sum(1 for e in events if e[0] == "validated" and e[3] == State.DONE)
  seen["restart"] = sum(1 for e in events if e[0] == "restart")
  return seen


def test_nonstop_captured_equals_online_adapter_steps(stream, monkeypatch):
  pairs, _ = stream
  fnet, snet = build()
  plain = OnlineAdapter(fnet, snet, H, W, lr=LR, fcs_ema_weight=EMA_WEIGHT)
  losses = []
  for i in range(STEPS):
    losses.append(float(plain.step(pairs[i][0].clone(), pairs[i][1].clone())["loss"]))
  loop, record, _ = _run("NONSTOP", True, stream, monkeypatch)
  assert loop.graph_count() == 1
  assert [r["loss"] for r in record] == losses
  assert all(r["updated"] == 1 and r["added"] == 0 for r in record)
  assert loop.gradient_updates == STEPS == loop.adapter.optimizer.step_count == plain.optimizer.step_count
  for a, b in ((plain.arena.params, loop.adapter.arena.params), (plain.optimizer.exp_avg, loop.adapter.optimizer.exp_avg),
               (plain.optimizer.exp_avg_sq, loop.adapter.optimizer.exp_avg_sq), (plain.fcs_smoothed, loop.adapter.fcs_smoothed)):
    assert torch.equal(a, b)
  for (n1, b1), (n2, b2) in zip(list(plain.stereo_net.named_buffers()) + list(plain.feature_net.named_buffers()),
                                list(loop.adapter.stereo_net.named_buffers()) + list(loop.adapter.feature_net.named_buffers())):
    assert n1 == n2 and torch.equal(b1, b2), n1


@pytest.mark.parametrize("mode", ["VS", "ER", "VS+ER"])
def test_captured_loop_equals_host_loop(mode, stream, monkeypatch):
  host, host_record, host_events = _run(mode, False, stream, monkeypatch)
  for i, r in enumerate(host_record):
    print(i, FAMILIES[i], BATCH_IDX[i], {k: (v.name if isinstance(v, State) else v) for k, v in r.items()})
  print(host_events)
  if mode != "ER":                       # (ER has no gate: nothing of this can happen)
    seen = _coverage(host_record, host_events, host)
    print(seen)
    assert all(v > 0 for v in seen.values()), seen
  dev, dev_record, dev_events = _run(mode, True, stream, monkeypatch)
  assert dev.graph_count() == 1
  assert host_events == dev_events
  for i, (a, b) in enumerate(zip(host_record, dev_record)):
    assert a == b, (i, a, b)
  _assert_same_words(_final_words(host), _final_words(dev))
  assert host.gradient_updates == dev.gradient_updates == sum(r["updated"] for r in host_record)
  assert host.adapter.optimizer.step_count == dev.adapter.optimizer.step_count == host.gradient_updates
  assert host.step == dev.step == STEPS and host.state_machine.state() == dev.state_machine.state()
  # the reservoirs: same size, same offers, same values, the same pairs in the same slots
  h, d = host.state_machine.ovs, dev.state_machine.ovs
  assert h.size() == d.size() and h.i == d.i
  for s in range(h.size()):
    hv, _, hl, hr = h.buf[s]
    dv, _, dl, dr = d.buf[s]
    assert float(hv) == float(dv) and torch.equal(hl, dl) and torch.equal(hr, dr), s
  if h.size():
    assert h.average_value() == d.average_value()
  sm_h, sm_d = host.state_machine, dev.state_machine
  assert (sm_h.prev_ovs_loss, sm_h.ovs_did_change, sm_h.ovs_iters_without_improvement) == \
         (sm_d.prev_ovs_loss, sm_d.ovs_did_change, sm_d.ovs_iters_without_improvement)


def test_in_progress_replay_does_not_synchronise(stream, monkeypatch):
  """Between two sync points an IN_PROGRESS step of the captured loop reads nothing back: no synchronising call is made, and
  the stream — given a few milliseconds of work just before the step — is still busy when process() returns."""
  calls = []
  for name in ("item", "cpu", "tolist", "__float__", "__int__", "__bool__"):
    orig = getattr(torch.Tensor, name)
    monkeypatch.setattr(torch.Tensor, name, (lambda o, n: lambda self, *a, **k: (calls.append(n), o(self, *a, **k))[1])(orig, name))
  for name in ("synchronize",):
    orig = getattr(torch.cuda, name)
    monkeypatch.setattr(torch.cuda, name, (lambda o, n: lambda *a, **k: (calls.append(n), o(*a, **k))[1])(orig, name))
  busy = []

  def after_step(loop, i, state_before):
    replayed = loop.graph_count() == 1 and i >= 3 and state_before == State.IN_PROGRESS and i % VALIDATE_HZ != 0
    if replayed and i % VALIDATE_HZ >= 2:
      busy.append(not torch.cuda.current_stream().query())
    after_step.sync_calls.append((i, replayed, list(calls)))
    del calls[:]
  after_step.sync_calls = []

  pairs, replay = stream
  loop = _loop("VS+ER", True, retries=1 << 20)             # never DONE: every step outside the sync points is a replay
  monkeypatch.setattr(control.random, "random", lambda: UNIFORMS[loop.step])
  filler = torch.rand(6144, 6144, device=DEV)
  for i in range(16):
    before = loop.state_machine.state()
    if i % VALIDATE_HZ >= 2:
      torch.mm(filler, filler)           # milliseconds of queued work: only a synchronising process() finds the stream idle after it
    loop.process(pairs[i][0], pairs[i][1], BATCH_IDX[i], replay=replay[i % len(replay)])
    after_step(loop, i, before)
  torch.cuda.synchronize()
  replays = [(i, c) for i, replayed, c in after_step.sync_calls if replayed]
  assert len(replays) >= 8
  assert all(c == [] for _, c in replays), replays
  assert busy and all(busy), busy


def test_captured_loop_refuses_a_data_parallel_adapter():
  class Dp(object):
    dp = True
  with pytest.raises(NotImplementedError):
    AdaptationLoop(Dp(), mode="VS", captured=True)
