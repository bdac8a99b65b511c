"""Adaptation on semi-global-matching proxy labels: OnlineAdapter(proxy_labeler=...), both AdaptationLoops, the validation metric
and adapt.py, on the geometry of tests/test_gpu_gated_loop.py (one pair, 64 x 96, k = 3, maxdisp 64, a labeler at D = 64).

On synthetic.stereo_pair(1, 64, 96, seed, disparities=(3.0 + seed % 5,)) the matcher's chain labels 0.94 - 0.97 of the pixels, on two
unrelated images 0.07 (computed on the CPU with the numpy chain for seeds 0, 1, 2, 7).  Every test that draws a conclusion from the
proxy term asserts, on the device's own count, a density of at least 0.9 on the shifted pairs it uses (DENSE) and a non-zero count
on the unrelated pair, so that nothing here rests on an empty label set unnoticed.

Equality is torch.equal on parameters, both Adam moments and every BatchNorm buffer: values, so +0.0 equals -0.0 (the gradient
g + 0.0 of an empty label set turns a -0.0 into +0.0 and nothing else)."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from adaptive_stereo import _native as nat
from adaptive_stereo import control, hip_ops
from adaptive_stereo.adaptation import OnlineAdapter
from adaptive_stereo.control import AdaptationLoop, State
from adaptive_stereo.sgm import ProxyLabeler
from adaptive_stereo.utils.loss_functions import khamis_robust_loss
import proxy_loss_ref as pl
import test_gpu_gated_loop as gl
from test_gpu_gated_loop import stream                     # noqa: F401  (the 40-step stream of the gated-loop test, a fixture)

DEV = gl.DEV
H, W, MAXDISP, LR = gl.H, gl.W, gl.MAXDISP, gl.LR
WEIGHT = 0.5
DENSE = 0.9


def labeler(**kwargs):
  return ProxyLabeler(H, W, batch=1, maxdisp=MAXDISP, **kwargs)


def adapter(lab=None, weight=WEIGHT, **kwargs):
  fnet, snet = gl.build()
  if lab is None:
    return OnlineAdapter(fnet, snet, H, W, lr=LR, fcs_ema_weight=gl.EMA_WEIGHT, **kwargs)
  return OnlineAdapter(fnet, snet, H, W, lr=LR, fcs_ema_weight=gl.EMA_WEIGHT, proxy_labeler=lab, proxy_loss_weight=weight, **kwargs)


def words(a):
  out = {"params": a.arena.params, "exp_avg": a.optimizer.exp_avg, "exp_avg_sq": a.optimizer.exp_avg_sq, "step_dev": a.optimizer.step_dev,
         "fcs_smoothed": a.fcs_smoothed}
  for tag, net in (("stereo_net", a.stereo_net), ("feature_net", a.feature_net)):
    for name, b in net.named_buffers():
      out["%s.%s" % (tag, name)] = b
  return {k: v.detach().clone() for k, v in out.items()}


def density(res):
  return float(res["proxy_count"]) / (H * W)


@pytest.fixture(scope="module")
def pairs():
  return [gl.familiar_pair(seed) for seed in (0, 1, 2, 7)]


# ================================================================================================================ the step
@pytest.mark.parametrize("proxy_only", [False, True], ids=["added", "proxy_only"])
def test_step_equals_the_step_composed_by_hand(proxy_only, pairs):
  """ProxyLabeler.__call__ -> khamis_robust_loss(pred, labels) -> loss + w * proxy -> backward -> FusedClipAdam, on a plain
  adapter's own arena, plan and optimizer, against OnlineAdapter.step with the labeler: three steps, bit for bit."""
  a = adapter(labeler(), proxy_only=proxy_only)
  b, lab_b = adapter(), labeler()
  for left, right in pairs[:3]:
    res = a.step(left.clone(), right.clone())
    assert density(res) >= DENSE, density(res)
    b.feature_net.train(); b.stereo_net.train()
    b.arena.rebind_grads(); b.arena.zero_grads()
    with hip_ops.step_region(b.plan, b.bn_sync):
      (loss, _, _), fcs_map, out, _warped, none = b._forward_maps(left.clone(), right.clone())
      assert none is None
      labels, _code, _counts = lab_b(left, right)
      proxy = khamis_robust_loss(out["pred_disp_l/0"], labels)
      (WEIGHT * proxy if proxy_only else loss + WEIGHT * proxy).backward()
    b.optimizer.step(clip=b.clip)
    b._update_fcs_ema(fcs_map.mean())
    assert torch.equal(res["loss"], loss.detach()) and torch.equal(res["proxy_loss"], proxy.detach())
    assert float(res["proxy_count"]) == float((labels > 0).sum())
    assert float(res["proxy_loss"]) > 0 and 0 < float(res["proxy_epe"]) and 0 <= float(res["proxy_bad"]) <= 1
  gl._assert_same_words(words(a), words(b))
  plain = adapter()
  for left, right in pairs[:3]:
    plain.step(left.clone(), right.clone())
  assert not torch.equal(plain.arena.params, a.arena.params)                # the term does something


def test_an_empty_label_set_is_the_photometric_step(pairs):
  a, plain = adapter(labeler(max_size=H * W)), adapter()                    # every component is a speckle: nothing is labelled
  for left, right in pairs[:3]:
    res = a.step(left.clone(), right.clone())
    want = plain.step(left.clone(), right.clone())
    assert float(res["proxy_count"]) == 0 and float(res["proxy_loss"]) == 0 and float(res["proxy_epe"]) == 0
    assert torch.equal(res["loss"], want["loss"])
  gl._assert_same_words(words(a), words(plain))


def test_unrelated_pair_still_carries_labels():
  a = adapter(labeler())
  left, right = gl.novel_pair(0)
  res = a.step(left, right)
  assert 0 < float(res["proxy_count"]) < DENSE * H * W


def test_captured_step_replays_eager_stepping(pairs):
  eager, cap = adapter(labeler()), adapter(labeler())
  own = labeler().capture()                                                 # a labeler with a graph of its own keeps it
  cap2 = adapter(own)
  first = pairs[0]
  for _ in range(3):
    eager.step(first[0].clone(), first[1].clone())
  cap.capture(first[0].clone(), first[1].clone(), warmup=3)
  cap2.capture(first[0].clone(), first[1].clone(), warmup=3)
  assert cap.graph_count() == 1 and cap2.graph_count() == 1 and own.captured()
  labels_before = own.labels_buffer().clone()
  for left, right in pairs[1:] + pairs[:2]:
    want = eager.step(left.clone(), right.clone())
    for c in (cap, cap2):
      got = c.step(left.clone(), right.clone())
      for key in ("loss", "proxy_loss", "proxy_epe", "proxy_bad", "proxy_count"):
        assert torch.equal(got[key], want[key]), key
    assert density(want) >= DENSE
  gl._assert_same_words(words(eager), words(cap))
  gl._assert_same_words(words(eager), words(cap2))
  assert torch.equal(own.labels_buffer(), labels_before)                    # the label map is not written on this path
  assert eager.optimizer.step_count == cap.optimizer.step_count == 8


def test_eval_mode_forwards_run_no_labeler(pairs):
  a = adapter(labeler())
  left, right = pairs[0]
  a.step(left.clone(), right.clone())
  calls = _recorded(lambda: a.forward_loss(left, right, train=False))[1]
  res = a.forward_loss(left, right, train=False)
  assert all(res[k] is None for k in ("proxy_loss", "proxy_epe", "proxy_bad", "proxy_count"))
  assert not [c for c in calls if c in NEW_CALLS]
  assert not [c for c in _recorded(lambda: a.infer(left, right))[1] if c in NEW_CALLS]


# ================================================================================================================ defaults
NEW_CALLS = ("as_sgm_census", "as_sgm_aggregate", "as_sgm_select", "as_lr_check", "as_disp_speckle", "as_proxy_term_fwd",
             "as_proxy_term_bwd")


def _recorded(fn):
  """fn() with every native call (adaptive_stereo._native.call, under both names it is bound to) recorded by name"""
  names = []
  original = nat.call

  def call(name, *args):
    names.append(name)
    return original(name, *args)
  nat.call = hip_ops.call = call
  try:
    result = fn()
  finally:
    nat.call = hip_ops.call = original
  return result, names


def test_defaults_enqueue_nothing_new(pairs):
  """Without a labeler (and with a labeler at weight 0) a step makes the native calls it made before, none of the labeler's or
  the node's; with one it makes exactly those in addition: two census launches, aggregate, select, the left-right check, the
  speckle pass, as_proxy_term_fwd and as_proxy_term_bwd."""
  left, right = pairs[0]
  lists = {}
  for name, make in (("plain", lambda: adapter()), ("weight 0", lambda: adapter(labeler(), weight=0.0)), ("active", lambda: adapter(labeler()))):
    a = make()
    a.step(left.clone(), right.clone())                                      # (the first step records the plan)
    lists[name] = _recorded(lambda: a.step(left.clone(), right.clone()))[1]
  assert len(lists["plain"]) > 50 and not [c for c in lists["plain"] if c in NEW_CALLS]
  assert lists["weight 0"] == lists["plain"]
  assert [c for c in lists["active"] if c not in NEW_CALLS] == lists["plain"]
  assert sorted(c for c in lists["active"] if c in NEW_CALLS) == sorted(NEW_CALLS + ("as_sgm_census",))
  # captured: one graph each, and the replays of the two agree bit for bit (the graphs' node lists themselves are not read here:
  # that they are the same is inferred from the equal call lists above, not measured)
  a, b = adapter(), adapter(labeler(), weight=0.0)
  a.capture(left.clone(), right.clone()); b.capture(left.clone(), right.clone())
  assert a.graph_count() == b.graph_count() == 1
  ra, rb = a.step(pairs[1][0].clone(), pairs[1][1].clone()), b.step(pairs[1][0].clone(), pairs[1][1].clone())
  assert torch.equal(ra["loss"], rb["loss"]) and rb["proxy_loss"] is None
  gl._assert_same_words(words(a), words(b))


# ================================================================================================================ the loops
def _run_loop(mode, captured, stream_, monkeypatch, steps=gl.STEPS, **loop_kwargs):
  pairs_, replay = stream_
  loop = AdaptationLoop(adapter(labeler()), mode=mode, ovs_buffer_size=gl.CAPACITY, ovs_validate_hz=gl.VALIDATE_HZ,
                        val_improve_retries=gl.RETRIES, ood_threshold=gl.THRESHOLD[mode], er_loss_weight=0.05, captured=captured,
                        **loop_kwargs)
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
  monkeypatch.setattr(gl.stereo_reservoir.random, "randint", lambda a, b: gl.randint_from_uniform(gl.UNIFORMS[loop.step], b))
  monkeypatch.setattr(control.random, "random", lambda: gl.UNIFORMS[loop.step])
  record = []
  for i in range(steps):
    before = sm.state()
    if i == gl.PUSH_STEP:
      loop.adapter.fcs_smoothed.fill_(gl.PUSH_VALUE)
    rep = replay[i % len(replay)] if mode in ("ER", "VS+ER") else None
    res = loop.process(pairs_[i][0].clone(), pairs_[i][1].clone(), gl.BATCH_IDX[i], replay=rep)
    opt = lambda key: None if res.get(key) is None else float(res[key])
    record.append(dict(family=gl.FAMILIES[i], state_before=before, state=res["state"], loss=float(res["loss"]), fcs=float(res["fcs"]),
                       fcs_smoothed=float(res["fcs_smoothed"]), updated=int(res["updated"]), added=int(res["added_to_ovs"]),
                       replay_loss=opt("replay_loss"), proxy_loss=opt("proxy_loss"), proxy_epe=opt("proxy_epe"),
                       proxy_bad=opt("proxy_bad"), proxy_count=opt("proxy_count")))
  loop.sync()
  torch.cuda.synchronize()
  return loop, record, events


@pytest.mark.parametrize("mode", ["VS", "VS+ER"])
def test_captured_loop_equals_host_loop_with_a_labeler(mode, stream, monkeypatch):            # noqa: F811
  host, host_record, host_events = _run_loop(mode, False, stream, monkeypatch)
  dev, dev_record, dev_events = _run_loop(mode, True, stream, monkeypatch)
  assert dev.graph_count() == 1
  assert host_events == dev_events
  for i, (a, b) in enumerate(zip(host_record, dev_record)):
    assert a == b, (i, a, b)
  gl._assert_same_words(words(host.adapter), words(dev.adapter))
  assert host.gradient_updates == dev.gradient_updates == sum(r["updated"] for r in host_record) > 0
  assert host.state_machine.state() == dev.state_machine.state()
  h, d = host.state_machine.ovs, dev.state_machine.ovs
  assert h.size() == d.size() and h.i == d.i
  for s in range(h.size()):
    assert float(h.buf[s][0]) == float(d.buf[s][0]) and torch.equal(h.buf[s][2], d.buf[s][2]), s
  # the label sets the run rests on: dense on the shifted pairs, present on the unrelated ones, absent only in eval-mode steps
  adapting = [r for r in host_record if r["proxy_count"] is not None]
  assert len(adapting) >= 20
  for r in adapting:
    assert r["proxy_count"] > 0 and r["proxy_loss"] > 0, r
    if r["family"] == "f":
      assert r["proxy_count"] >= DENSE * H * W, r
  # a step without the term is an eval-mode step (the machine was DONE before it, or the validation at its start made it so,
  # whatever the gate then did): it never updates
  for r in host_record:
    if r["proxy_count"] is None:
      assert r["updated"] == 0, r
    else:
      assert r["state_before"] == State.IN_PROGRESS, r
  if mode == "VS+ER":
    assert all(r["replay_loss"] is not None for r in host_record)


def test_replayed_step_with_a_labeler_does_not_synchronise(stream, monkeypatch):              # noqa: F811
  calls = []
  for name in ("item", "cpu", "tolist", "__float__", "__int__", "__bool__"):
    orig = getattr(torch.Tensor, name)
    monkeypatch.setattr(torch.Tensor, name, (lambda o, n: lambda self, *a, **k: (calls.append(n), o(self, *a, **k))[1])(orig, name))
  orig_sync = torch.cuda.synchronize
  monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.append("synchronize"), orig_sync(*a, **k))[1])
  pairs_, replay = stream
  loop = AdaptationLoop(adapter(labeler()), mode="VS+ER", ovs_buffer_size=gl.CAPACITY, ovs_validate_hz=gl.VALIDATE_HZ,
                        val_improve_retries=1 << 20, ood_threshold=gl.THRESHOLD["VS+ER"], captured=True)
  monkeypatch.setattr(control.random, "random", lambda: gl.UNIFORMS[loop.step])
  seen = []
  for i in range(12):
    before = loop.state_machine.state()
    loop.process(pairs_[i][0], pairs_[i][1], gl.BATCH_IDX[i], replay=replay[i % len(replay)])
    replayed = loop.graph_count() == 1 and i >= 3 and before == State.IN_PROGRESS and i % gl.VALIDATE_HZ != 0
    seen.append((i, replayed, list(calls)))
    del calls[:]
  orig_sync()
  replays = [(i, c) for i, replayed, c in seen if replayed]
  assert len(replays) >= 6
  assert all(c == [] for _, c in replays), replays


# ================================================================================================================ the validation metric
def test_ovs_metric_proxy_epe(pairs):
  lab = labeler()
  a = adapter(lab)
  loop = AdaptationLoop(a, mode="VS", ovs_buffer_size=3, ovs_validate_hz=2, val_improve_retries=1 << 20, ood_threshold=1e30,
                        ovs_metric="proxy_epe")
  for i, (left, right) in enumerate(pairs):
    loop.process(left.clone(), right.clone(), i)
  ovs = loop.state_machine.ovs
  assert ovs.size() == 3
  received = []
  loop.state_machine.validate(lambda l, r: received.append(loop._validation_loss(l, r)) or received[-1])
  assert len(received) == 3
  for s in range(3):
    value, _, left, right = ovs.buf[s]
    assert received[s] == a.validation_proxy_epe(left, right) == float(value)
    # ... which is the reference's mean |matcher - network| on the eval-mode prediction and the labeler's outputs
    a.feature_net.eval(); a.stereo_net.eval()
    with torch.no_grad():
      fl, fr = a._features_eval(left, right)
      pred = a.stereo_net(left, fl, fr, "l", output_cost_volume=True)["pred_disp_l/0"].cpu().numpy()
    a.feature_net.train(); a.stereo_net.train()
    disp, code, _ = lab.chain(left, right)
    ref = pl.forward(pred, disp.cpu().numpy(), code.cpu().numpy(), 3.0)
    assert ref[5] >= DENSE * H * W
    m, _v, e = pl.pixel_terms(pred, disp.cpu().numpy(), code.cpu().numpy())
    exact = math.fsum(e[m].astype(np.float64).tolist()) / int(m.sum())
    assert abs(received[s] - exact) <= float(np.spacing(np.float32(exact))), (received[s], exact)
    assert received[s] != a.validation_loss(left, right)
  assert a.feature_net.training and a.stereo_net.training                    # the modes are put back
  # a pair without a single label scores by its photometric loss
  empty = adapter(labeler(max_size=H * W))
  left, right = pairs[0]
  assert empty.validation_proxy_epe(left, right) == empty.validation_loss(left, right) > 0
  assert "0.0" in OnlineAdapter.validation_proxy_epe.__doc__ and "photometric" in OnlineAdapter.validation_proxy_epe.__doc__


# ================================================================================================================ refusals
def test_refusals(monkeypatch):
  import torch.distributed as dist
  fnet, snet = gl.build()
  lab = labeler()
  with pytest.raises(ValueError, match="proxy_only"):
    OnlineAdapter(fnet, snet, H, W, proxy_only=True)
  with pytest.raises(ValueError, match="proxy_only"):
    OnlineAdapter(fnet, snet, H, W, proxy_labeler=lab, proxy_only=True)           # weight 0
  with pytest.raises(ValueError, match="negative"):
    OnlineAdapter(fnet, snet, H, W, proxy_labeler=lab, proxy_loss_weight=-0.5)
  with pytest.raises(ValueError, match="without a proxy_labeler"):
    OnlineAdapter(fnet, snet, H, W, proxy_loss_weight=0.5)
  with pytest.raises(ValueError, match="proxy_bad_px"):
    OnlineAdapter(fnet, snet, H, W, proxy_labeler=lab, proxy_loss_weight=0.5, proxy_bad_px=float("nan"))
  with pytest.raises(ValueError, match="64 x 96"):
    OnlineAdapter(fnet, snet, H, W, proxy_labeler=ProxyLabeler(H, W + 32, maxdisp=MAXDISP), proxy_loss_weight=0.5)
  two = OnlineAdapter(fnet, snet, H, W, proxy_labeler=ProxyLabeler(H, W, batch=2, maxdisp=MAXDISP), proxy_loss_weight=0.5)
  left, right = gl.familiar_pair(0)
  with pytest.raises(ValueError, match="batch of 1"):
    two.step(left, right)
  with pytest.raises(ValueError, match="proxy_labeler"):
    AdaptationLoop(OnlineAdapter(fnet, snet, H, W), mode="VS", ovs_metric="proxy_epe")
  with pytest.raises(RuntimeError, match="proxy_labeler"):
    OnlineAdapter(fnet, snet, H, W).validation_proxy_epe(left, right)
  # data parallel: what the constructor asks torch.distributed, answered as in a group of two ranks
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
  with pytest.raises(NotImplementedError, match="data-parallel"):
    OnlineAdapter(fnet, snet, H, W, native_collectives=False, proxy_labeler=lab, proxy_loss_weight=0.5)
  assert OnlineAdapter(fnet, snet, H, W, native_collectives=False).dp


# ================================================================================================================ the command line
def test_adapt_command_line(tmp_path):
  """adapt() on injected datasets with --proxy_loss_weight 0.5: the captured loop and --no_capture end at the same weights, opt.json
  carries the options, the Proxy/ scalars are logged; --proxy_loss_weight 0 ends where a run without the option ends."""
  import adapt as adapt_module
  import test_gpu_adapt_cli as cli
  stream_, adapt_val, train_val = cli._samples(5, 3), cli._samples(6, 2), cli._samples(7, 2)
  folder = cli._weights_folder(tmp_path / "pretrained")

  class Writer(object):
    def __init__(self):
      self.scalars = []

    def add_scalar(self, name, value, step):
      self.scalars.append((name, step, float(value)))

    def add_image(self, name, image, step):
      pass

  def run(name, *extra):
    writer = Writer()
    opt = cli._options(tmp_path, folder, "--model_name", name, "--skip_initial_eval", *extra)
    loop = adapt_module.adapt(opt, cli.ListDataset(stream_), cli.ListDataset(adapt_val), cli.ListDataset(train_val), writer=writer)
    return loop, writer, json.load(open(os.path.join(str(tmp_path), name, "opt.json")))

  proxy = ("--proxy_loss_weight", "0.5", "--proxy_paths", "4", "--proxy_max_size", "100", "--ovs_metric", "proxy_epe")
  cap, writer, saved = run("captured", *proxy)
  host, _, _ = run("host", "--no_capture", *proxy)
  assert cap.captured and cap.graph_count() == 1 and not host.captured
  assert cap.gradient_updates == host.gradient_updates == 3
  assert (saved["proxy_loss_weight"], saved["proxy_only"], saved["proxy_paths"], saved["proxy_uniqueness"], saved["proxy_max_size"],
          saved["ovs_metric"]) == (0.5, False, 4, 5, 100, "proxy_epe")
  lab = cap.adapter.proxy_labeler
  assert (lab.matcher.H, lab.matcher.W, lab.matcher.B, lab.matcher.D, lab.matcher.paths, lab.filter.max_size) == (cli.H, cli.W, 1, 192, 4, 100)
  assert cap.ovs_metric == "proxy_epe"
  gl._assert_same_words(words(cap.adapter), words(host.adapter))
  logged = {name: value for name, step, value in writer.scalars if step == 4}
  assert {"Proxy/loss", "Proxy/epe", "Proxy/bad", "Proxy/density"} <= set(logged)
  assert 0 < logged["Proxy/density"] <= 1 and logged["Proxy/loss"] > 0
  rows = adapt_module.read_trials(os.path.join(str(tmp_path), "captured", "trials.csv"))
  assert tuple(rows[0].keys()) == adapt_module.TRIALS_COLUMNS

  zero, zero_writer, _ = run("zero", "--proxy_loss_weight", "0")
  none, _, saved_none = run("none")
  assert zero.adapter.proxy_labeler is None and saved_none["proxy_loss_weight"] == 0.0
  gl._assert_same_words(words(zero.adapter), words(none.adapter))
  assert not torch.equal(none.adapter.arena.params, cap.adapter.arena.params)
  assert not [s for s in zero_writer.scalars if s[0].startswith("Proxy/")]
