"""tests/proxy_loss_ref.py, the numpy restatement the GPU tests hold csrc/proxy_loss.hip to, pinned without a GPU: against torch
fp64 (KhamisLossFn's formula and autograd) on the label set, against cases worked by hand, and against four plausible mistakes
(proxy_loss_ref.WRONG), each of which a named case tells from the contract.  Then the host side: the entry points are declared and
bound, and every refusal comes before the first HIP call."""
import numpy as np
import pytest
import torch

import proxy_loss_ref as pl

F = np.float32
NAN, INF = F(np.nan), F(np.inf)


def bits(a):
  return np.asarray(a, dtype=F).view(np.uint32)


# ------------------------------------------------------------------------------------------------- against torch fp64
@pytest.mark.parametrize("n,seed", [(1, 0), (65, 1), (4099, 2)])
def test_forward_and_backward_against_torch_fp64(n, seed):
  pred, disp, code = pl.planted_case(n, seed)
  if n == 1:
    disp[0], code[0] = F(7.5), 0
  out6 = pl.forward(pred, disp, code, 3.0)
  m = pl.labelled(disp, code)
  assert np.array_equal(m, pl.materialised_labels(disp, code) > 0)                 # the set the supervised path sees
  p = torch.tensor(pred.astype(np.float64), requires_grad=True)
  g = torch.tensor(np.where(m, disp, 0).astype(np.float64))
  mask = torch.tensor(m)
  # utils/loss_functions.py:6-15 (KhamisLossFn's formula) in fp64
  loss = (torch.sqrt((g - p) ** 2 + 4.0) / 2.0 - 1.0)[mask].sum() / max(int(m.sum()), 1)
  loss.backward()
  loss, q = loss.detach(), p.detach()
  count = int(m.sum())
  assert out6[5] == count and out6[1] == max(count, 1)
  # per pixel the fp32 chain carries about 2.5 ulps of values up to d^2/...: a relative 2^-20 on the mean covers every shape here
  assert abs(float(out6[0]) - float(loss)) <= 2.0 ** -20 * max(abs(float(loss)), 1.0)
  epe = float((g - q).abs()[mask].sum() / max(count, 1))
  assert abs(float(out6[3]) - epe) <= 2.0 ** -22 * max(epe, 1.0)
  bad = float(((g - q).abs()[mask] > 3.0).sum()) / max(count, 1)
  assert abs(float(out6[4]) - bad) <= 2.0 / max(count, 1) + 1e-7        # (a pixel within an fp32 rounding of 3.0 may fall either way)
  g64 = pl.backward64(pred, disp, code, 0.75)
  assert np.allclose(g64, 0.75 * p.grad.numpy(), rtol=1e-12, atol=0)
  g32 = pl.backward(pred, disp, code, 0.75, out6)
  assert g32.dtype == F and np.all(bits(g32[~m]) == 0)                              # exactly +0.0 off the label set
  assert np.all(np.abs(g32.astype(np.float64) - g64) <= 2.0 ** -21 * np.abs(g64) + 1e-42)


# ------------------------------------------------------------------------------------------------- by hand
def test_no_label_at_all():
  pred = np.array([1.0, 2.0, 3.0, 4.0], dtype=F)
  out6 = pl.forward(pred, [0.0, -1.0, 5.0, np.nan], [0, 0, 3, 0], 3.0)
  assert out6.tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
  assert np.all(bits(pl.backward(pred, [0.0, -1.0, 5.0, np.nan], [0, 0, 3, 0], 1.0, out6)) == 0)


def test_one_label_by_hand():
  # d = 3: sqrt(13) / 2 - 1; one pixel in five carries it
  out6 = pl.forward([9.0, 5.0, 9.0, 9.0, 9.0], [9.0, 8.0, 9.0, 9.0, 9.0], [1, 0, 2, 6, 7], 2.5)
  v = F(F(np.sqrt(F(13.0))) / F(2)) - F(1)
  assert out6.tolist() == [float(v), 1.0, float(v), 3.0, 1.0, 1.0]
  g = pl.backward([9.0, 5.0, 9.0, 9.0, 9.0], [9.0, 8.0, 9.0, 9.0, 9.0], [1, 0, 2, 6, 7], 2.0, out6)
  want = F(F(-2.0) * F(3.0)) / F(F(2) * F(np.sqrt(F(13.0))))
  assert g.tolist() == [0.0, float(want), 0.0, 0.0, 0.0]
  # two labels: the mean of both; the unlabelled prediction does not matter, NaN included
  out6 = pl.forward([1.0, NAN, 4.0], [1.0, 5.0, 8.0], [0, 5, 0], 3.0)
  v4 = F(F(np.sqrt(F(20.0))) / F(2)) - F(1)
  assert out6.tolist() == [float(F(v4) / F(2)), 2.0, float(v4), 2.0, 0.5, 2.0]


def test_bad_px_exactly_and_its_neighbours():
  bad_px = F(3.0)
  below, above = np.nextafter(bad_px, F(0)), np.nextafter(bad_px, F(10))
  pred = np.zeros(3, dtype=F)
  disp = np.array([below, bad_px, above], dtype=F)                 # |e| = the disparity itself, exactly
  for k, share in ((0, 0.0), (1, 0.0), (2, 1.0)):                  # strictly greater: |e| == bad_px is not bad
    assert pl.forward(pred[k:k + 1], disp[k:k + 1], [0], bad_px)[4] == share, k
  assert pl.forward(pred, disp, [0, 0, 0], bad_px)[4] == F(1.0 / 3.0)
  assert pl.forward(pred, disp, [0, 0, 0], 0.0)[4] == 1.0 and pl.forward(pred, pred + F(1), [0, 0, 0], 1.0)[4] == 0.0


def test_code_zero_with_unusable_disparities_and_infinity():
  pred = np.full(5, 2.0, dtype=F)
  disp = np.array([NAN, -0.0, 0.0, -3.0, INF], dtype=F)
  assert pl.labelled(disp, np.zeros(5, np.uint8)).tolist() == [False, False, False, False, True]
  assert pl.forward(pred[:4], disp[:4], np.zeros(4, np.uint8), 3.0).tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
  out6 = pl.forward(pred, disp, np.zeros(5, np.uint8), 3.0)        # +inf > 0 is a label, as where(code == 0, disp, 0) > 0 has it
  assert out6[5] == 1 and np.isinf(out6[0]) and np.isinf(out6[3]) and out6[4] == 1.0
  assert np.array_equal(pl.labelled(disp, np.zeros(5, np.uint8)), pl.materialised_labels(disp, np.zeros(5, np.uint8)) > 0)


def test_every_non_zero_code_carries_no_label():
  codes = np.arange(1, 8, dtype=np.uint8)
  disp = np.full(7, 5.0, dtype=F)
  assert not pl.labelled(disp, codes).any()
  assert pl.forward(np.zeros(7, F), disp, codes, 3.0).tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
  for k in range(7):                                               # ... and each one alone beside a label
    out6 = pl.forward([0.0, 0.0], [5.0, 5.0], [codes[k], 0], 3.0)
    assert out6[5] == 1 and out6[3] == 5.0
  assert pl.forward(np.zeros(2, F), [5.0, 5.0], [255, 128], 3.0)[5] == 0


# ------------------------------------------------------------------------------------------------- wrong restatements
def test_wrong_restatements_are_caught():
  right = lambda *a: pl.forward(*a)
  differs = lambda wrong, *a: not np.array_equal(bits(pl.forward(*a, wrong=wrong)), bits(right(*a)))
  caught = {
    "bad_ge": differs("bad_ge", [0.0], [3.0], [0], 3.0),                                   # |e| == bad_px
    "disp_ge_zero": differs("disp_ge_zero", [1.0, 1.0], [0.0, 4.0], [0, 0], 3.0),          # disp == 0 under code 0
    "ignore_code": differs("ignore_code", [1.0, 1.0], [6.0, 4.0], [6, 0], 3.0),            # a speckle with a positive disparity
    "raw_count_denominator": differs("raw_count_denominator", [1.0], [6.0], [4], 3.0),     # no label: 0 / 0
  }
  assert set(caught) == set(pl.WRONG)
  assert all(caught.values()), caught
  # and none of them differs where its case does not arise
  pred, disp, code = np.array([1.0, 2.0], F), np.array([2.5, 4.0], F), np.zeros(2, np.uint8)
  for wrong in pl.WRONG:
    assert not differs(wrong, pred, disp, code, 3.0), wrong


# ------------------------------------------------------------------------------------------------- the host side
def test_entry_points_are_declared_and_bound():
  from adaptive_stereo import _native as nat
  lib = nat.load()
  for name in ("as_proxy_term_workspace", "as_proxy_term_fwd", "as_proxy_term_bwd"):
    assert name in nat.EXPORTED_SYMBOLS and hasattr(lib, name)
  assert lib.as_proxy_term_workspace(1) == lib.as_proxy_term_workspace(1 << 31) == 2 * lib.as_khamis_workspace(1) == 4096
  assert lib.as_proxy_term_workspace(0) == -1 and lib.as_proxy_term_workspace(-5) == -1
  from adaptive_stereo import hip_ops
  assert hasattr(hip_ops, "ProxyTermFn")


def test_refusals_before_any_launch():
  """every argument check returns before the first HIP call, so it runs without a GPU"""
  import ctypes
  import re
  from adaptive_stereo import _native as nat
  lib = nat.load()
  vp = ctypes.c_void_p
  p, d, c, o, w, g, q = vp(1 << 16), vp(1 << 17), vp(1 << 18), vp(1 << 19), vp(1 << 20), vp(1 << 21), vp(1 << 22)   # never dereferenced
  nan, inf = float("nan"), float("inf")
  cases = [
    ("as_proxy_term_fwd", (None, d, c, 8, 3.0, o, w, None), "null"),
    ("as_proxy_term_fwd", (p, None, c, 8, 3.0, o, w, None), "null"),
    ("as_proxy_term_fwd", (p, d, None, 8, 3.0, o, w, None), "null"),
    ("as_proxy_term_fwd", (p, d, c, 8, 3.0, None, w, None), "null"),
    ("as_proxy_term_fwd", (p, d, c, 8, 3.0, o, None, None), "null"),
    ("as_proxy_term_fwd", (p, d, c, 0, 3.0, o, w, None), "positive"),
    ("as_proxy_term_fwd", (p, d, c, -4, 3.0, o, w, None), "positive"),
    ("as_proxy_term_fwd", (p, d, c, 8, 3.0, o, vp((1 << 20) + 4), None), "8-byte"),
    ("as_proxy_term_fwd", (vp((1 << 16) + 2), d, c, 8, 3.0, o, w, None), "4-byte"),
    ("as_proxy_term_fwd", (p, d, c, 8, -1.0, o, w, None), "bad_px"),
    ("as_proxy_term_fwd", (p, d, c, 8, nan, o, w, None), "bad_px"),
    ("as_proxy_term_fwd", (p, d, c, 8, inf, o, w, None), "bad_px"),
    ("as_proxy_term_fwd", (p, d, c, 8, 3.0, vp((1 << 16) + 28), w, None), "alias"),          # out6 inside pred
    ("as_proxy_term_fwd", (p, d, c, 8, 3.0, vp((1 << 18) + 4), w, None), "alias"),           # out6 inside code
    ("as_proxy_term_fwd", (p, d, c, 8, 3.0, o, vp((1 << 19) + 16), None), "alias"),          # the workspace over out6
    ("as_proxy_term_fwd", (p, d, c, 8, 3.0, o, vp((1 << 17) - 4096 * 4 + 8), None), "alias"),  # the workspace running into disp
    ("as_proxy_term_bwd", (None, d, c, q, o, 8, g, None), "null"),
    ("as_proxy_term_bwd", (p, None, c, q, o, 8, g, None), "null"),
    ("as_proxy_term_bwd", (p, d, None, q, o, 8, g, None), "null"),
    ("as_proxy_term_bwd", (p, d, c, None, o, 8, g, None), "null"),
    ("as_proxy_term_bwd", (p, d, c, q, None, 8, g, None), "null"),
    ("as_proxy_term_bwd", (p, d, c, q, o, 8, None, None), "null"),
    ("as_proxy_term_bwd", (p, d, c, q, o, 0, g, None), "positive"),
    ("as_proxy_term_bwd", (p, d, c, q, o, 8, vp((1 << 21) + 1), None), "4-byte"),
    ("as_proxy_term_bwd", (p, d, c, q, o, 8, p, None), "alias"),                              # in place over pred
    ("as_proxy_term_bwd", (p, d, c, q, o, 8, vp((1 << 17) + 28), None), "alias"),            # over the last element of disp
    ("as_proxy_term_bwd", (p, d, c, q, o, 8, vp((1 << 18) - 28), None), "alias"),            # running into code
    ("as_proxy_term_bwd", (p, d, c, q, o, 8, vp((1 << 19) + 20), None), "alias"),            # over out6
    ("as_proxy_term_bwd", (p, d, c, q, o, 8, vp((1 << 22) - 28), None), "alias"),            # running into g_loss
  ]
  for name, args, word in cases:
    assert getattr(lib, name)(*args) == -1, (name, args)
    assert re.search(word, lib.as_last_error().decode()), (name, word, lib.as_last_error())


def test_python_side_refusals_without_a_gpu():
  from adaptive_stereo import hip_ops
  from adaptive_stereo.control import AdaptationLoop, OVS_METRICS

  class NoLabeler(object):
    dp = False
    proxy_labeler = None
  assert OVS_METRICS == ("photometric", "proxy_epe")
  with pytest.raises(ValueError, match="proxy_labeler"):
    AdaptationLoop(NoLabeler(), mode="VS", ovs_metric="proxy_epe")
  with pytest.raises(ValueError, match="ovs_metric"):
    AdaptationLoop(NoLabeler(), mode="VS", ovs_metric="epe")
  assert AdaptationLoop(NoLabeler(), mode="VS").ovs_metric == "photometric"
  with pytest.raises(RuntimeError, match="no CPU path|GPU"):
    hip_ops.ProxyTermFn.apply(torch.zeros(4), torch.zeros(4), torch.zeros(4, dtype=torch.uint8), 3.0)


def test_command_line_options():
  import adapt as adapt_module
  import train as train_module
  opt = train_module.TrainOptions().parse([])
  assert (opt.proxy_loss_weight, opt.proxy_only, opt.proxy_paths, opt.proxy_uniqueness, opt.proxy_max_size, opt.ovs_metric) == \
         (0.0, False, 8, 5, 200, "photometric")
  opt = train_module.TrainOptions().parse(["--proxy_loss_weight", "0.5", "--proxy_only", "--proxy_paths", "4", "--proxy_uniqueness",
                                           "10", "--proxy_max_size", "50", "--ovs_metric", "proxy_epe"])
  assert (opt.proxy_loss_weight, opt.proxy_only, opt.proxy_paths, opt.proxy_uniqueness, opt.proxy_max_size, opt.ovs_metric) == \
         (0.5, True, 4, 10, 50, "proxy_epe")
  with pytest.raises(SystemExit):
    train_module.TrainOptions().parse(["--proxy_paths", "6"])
  assert adapt_module.proxy_labeler_from_options(train_module.TrainOptions().parse([]), None) is None
  for flags in (["--proxy_only"], ["--ovs_metric", "proxy_epe"]):
    with pytest.raises(ValueError, match="proxy_loss_weight"):
      adapt_module.proxy_labeler_from_options(train_module.TrainOptions().parse(flags), None)

  class Net(object):
    maxdisp = 320
  with pytest.raises(ValueError, match="256"):
    adapt_module.proxy_labeler_from_options(train_module.TrainOptions().parse(["--proxy_loss_weight", "1"]), Net())
